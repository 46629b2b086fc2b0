"""ABI 51 without a GPU: the version in the header, the library and _lib.py; the ctypes mirror of
regnn_ns_csc_job against the header's members; the rank job's and regnn_ns_hop's refusals
(returned before anything is launched, so fake non-NULL pointers do)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = 1, 2
_SIZE = {"int32_t": 4}


def _job_members():
    src = open(os.path.join(ROOT, "include", "regnn_hip.h")).read()
    body = re.search(r"typedef struct regnn_ns_csc_job \{(.*?)\} regnn_ns_csc_job;", src,
                     re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [s.strip() for s in body.split(";") if s.strip()]


def test_abi_50_everywhere():
    from regnn_hip import _lib, build
    assert _lib._so.regnn_abi_version() == _lib.ABI_VERSION == build.header_abi() == 51


def test_csc_job_mirror_has_the_headers_layout():
    from regnn_hip import ns
    members = _job_members()
    fields = ns._NsCscJob._fields_
    assert [m.split()[-1].lstrip("*") for m in members] == [f[0] for f in fields]
    assert members[-2:] == ["int32_t* csc_cnt", "int32_t* csc_rank"]
    size = align = 0
    for m, (_, ct) in zip(members, fields):
        n = 8 if "*" in m else _SIZE[m.split()[0]]
        assert ctypes.sizeof(ct) == n, m
        size = (size + n - 1) // n * n + n
        align = max(align, n)
    assert ctypes.sizeof(ns._NsCscJob) == (size + align - 1) // align * align == 48
    assert [getattr(ns._NsCscJob, f[0]).offset for f in fields] == [0, 4, 8, 16, 24, 32, 40]


def _sums_call(job, hop=1):
    """regnn_ns_hop_typed_sums with valid-looking arguments (never dereferenced on the host
    except the table array) and the given job"""
    from regnn_hip import _lib
    fake = 0x10000
    tabs = (ctypes.c_void_p * 4)(fake, fake, fake, fake)
    return _lib._so.regnn_ns_hop_typed_sums(
        fake, fake, fake, fake, 7, 5, hop, fake, fake, fake, 64, fake, fake, fake, fake, fake,
        fake, tabs, 4, 128, fake, fake, fake, fake, ctypes.addressof(job), None, None)


def _job(cap_e, **null):
    """a job of hop 0 with fake pointers; the members named in `null` (as name=None) NULL"""
    from regnn_hip import ns
    ptrs = dict.fromkeys(("gsrc", "g2l", "blk_idx", "csc_cnt", "csc_rank"), 0x10000)
    assert set(null) <= set(ptrs)
    return ns._NsCscJob(0, cap_e, **{**ptrs, **null})


def test_rank_job_refusals():
    assert _sums_call(_job(32768 + 1)) == EUNSUPPORTED         # past kCscMax
    assert _sums_call(_job(4096, csc_rank=None)) == EINVAL     # a job without csc_rank
    assert _sums_call(_job(4096, gsrc=None)) == EINVAL
    assert _sums_call(_job(4096, csc_cnt=None)) == EINVAL
    assert _sums_call(_job(4096), hop=0) == EINVAL             # the job's hop is not earlier


def _hop_call(strided, rank, local=None, meta_only=0, csc=0x10000):
    """regnn_ns_hop of hop 0 with fake pointers: csc = the four index buffers, local = the edge
    meta's three"""
    from regnn_hip import _lib
    f = 0x10000
    return _lib._so.regnn_ns_hop(f, f, f, f, 7, 5, 0, f, f, f, 64, f, f, f, f, f, f, f, f, f, f,
                                 f, f, f, f, f, local, local, local, meta_only, csc, csc, csc, csc,
                                 rank, strided, None)


def test_hop_modes_refused_before_any_launch():
    """ABI 51: strided = 3 (the removed one-launch build) and a strided index without edge meta
    and without csc_rank; strided = 4 (first half only) as before"""
    f = 0x10000
    assert _hop_call(3, f) == EINVAL
    assert _hop_call(3, None) == EINVAL
    assert _hop_call(1, None) == EINVAL
    assert _hop_call(4, None) == EINVAL
    assert _hop_call(4, f, local=f) == EINVAL                  # with edge meta
    assert _hop_call(4, f, csc=None) == EINVAL                 # without the index buffers


def test_placement_only_mode_needs_the_split_buffers():
    """regnn_ns_hop strided = 5 (placement only): refused without csc_rank, with edge meta, or
    meta-only"""
    f = 0x10000
    assert _hop_call(5, None) == EINVAL
    assert _hop_call(5, f, local=f) == EINVAL
    assert _hop_call(5, f, local=f, meta_only=1) == EINVAL
    assert _hop_call(5, f, csc=None) == EINVAL
