"""ABI 50 without a GPU: the version in the header, the library and _lib.py; the ctypes mirror of
regnn_ns_csc_job against the header's members; the rank job's refusals (returned before anything
is launched, so fake non-NULL pointers do)."""
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
    assert _lib._so.regnn_abi_version() == _lib.ABI_VERSION == build.header_abi() == 50


def test_csc_job_mirror_has_the_headers_layout():
    from regnn_hip import ns
    members = _job_members()
    fields = ns._NsCscJob._fields_
    assert [m.split()[-1].lstrip("*") for m in members] == [f[0] for f in fields]
    assert members[-2:] == ["int32_t* csc_rank", "int32_t kind"]     # appended at the end
    size = align = 0
    for m, (_, ct) in zip(members, fields):
        n = 8 if "*" in m else _SIZE[m.split()[0]]
        assert ctypes.sizeof(ct) == n, m
        size = (size + n - 1) // n * n + n
        align = max(align, n)
    assert ctypes.sizeof(ns._NsCscJob) == (size + align - 1) // align * align == 104
    assert ns._NsCscJob.csc_rank.offset == 88 and ns._NsCscJob.kind.offset == 96


def _sums_call(job, hop=1):
    """regnn_ns_hop_typed_sums with valid-looking arguments (never dereferenced on the host
    except the table array) and the given job"""
    from regnn_hip import _lib
    fake = 0x10000
    tabs = (ctypes.c_void_p * 4)(fake, fake, fake, fake)
    return _lib._so.regnn_ns_hop_typed_sums(
        fake, fake, fake, fake, 7, 5, hop, fake, fake, fake, 64, fake, fake, fake, fake, fake,
        fake, tabs, 4, 128, fake, fake, fake, fake, ctypes.addressof(job), None, None)


def _job(cap_e, kind, rank=0x10000):
    from regnn_hip import ns
    f = 0x10000
    return ns._NsCscJob(0, cap_e, f, f, f, f, f, f, f, f, f, f, rank, kind)


def test_rank_job_refusals():
    assert _sums_call(_job(32768 + 1, 1)) == EUNSUPPORTED      # past kCscMax
    assert _sums_call(_job(32768 + 1, 0)) == EUNSUPPORTED
    assert _sums_call(_job(4096, 1, rank=None)) == EINVAL      # a rank job without csc_rank
    assert _sums_call(_job(4096, 2)) == EINVAL                 # no such kind
    assert _sums_call(_job(4096, 1), hop=0) == EINVAL          # the job's hop is not earlier


def test_placement_only_mode_needs_the_split_buffers():
    """regnn_ns_hop strided = 5 (placement only): refused without csc_rank, with edge meta, or
    meta-only"""
    from regnn_hip import _lib
    f = 0x10000
    hop = _lib._so.regnn_ns_hop

    def call(rank, local=None, meta_only=0, csc=f):
        return hop(f, f, f, f, 7, 5, 0, f, f, f, 64, f, f, f, f, f, f, f, f, f, f, f, f, f, f, f,
                   local, local, local, meta_only, csc, csc, csc, csc, rank, 5, None)
    assert call(None) == EINVAL
    assert call(f, local=f) == EINVAL
    assert call(f, local=f, meta_only=1) == EINVAL
    assert call(f, csc=None) == EINVAL
