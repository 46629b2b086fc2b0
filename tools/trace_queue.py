"""One queue's per-batch timeline in a rocprofv3 kernel trace: each launch's mean duration and the
mean idle gap before it on its own queue (start minus the end of the queue's previous dispatch).

usage: trace_queue.py TRACE_CSV MARKER K
The queue is the one the dispatches whose name contains MARKER run on (the first launch of a
batch's chain, e.g. ns_batch_kernel or ns_sample_strided); the window is the last K whole chains
(from the (K+1)-th last marker to the last one). Prints per launch (in chain order) the mean
duration and gap, then the chain's kernel time, its gaps and its length first start to last end
(the longest wait inside it, typically the sums launch's wait for the model step, listed apart)."""
import csv
import sys
from collections import defaultdict


def main():
    path, marker, k = sys.argv[1], sys.argv[2], int(sys.argv[3])
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    qkey = "Queue_Id" if "Queue_Id" in rows[0] else "Stream_Id"
    marks = [r for r in rows if marker in r["Kernel_Name"]]
    if len(marks) < k + 1:
        raise SystemExit(f"only {len(marks)} '{marker}' dispatches")
    q = marks[-1][qkey]
    rows = [r for r in rows if r[qkey] == q]
    starts = [i for i, r in enumerate(rows) if marker in r["Kernel_Name"]]
    dur, gap, cnt, order = defaultdict(float), defaultdict(float), defaultdict(int), []
    length = kern = 0.0
    for a, b in zip(starts[-k - 1:-1], starts[-k:]):
        chain = rows[a:b]
        for j, r in enumerate(chain):
            s, e = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
            name = r["Kernel_Name"].split("(")[0][:60]
            if name not in cnt:
                order.append(name)
            prev = int(rows[a + j - 1]["End_Timestamp"]) if a + j > 0 else s
            dur[name] += (e - s) / 1e3
            gap[name] += (s - prev) / 1e3
            cnt[name] += 1
            kern += (e - s) / 1e3
        length += (int(chain[-1]["End_Timestamp"]) - int(chain[0]["Start_Timestamp"])) / 1e3
    period = (int(rows[starts[-1]]["Start_Timestamp"]) -
              int(rows[starts[-k - 1]]["Start_Timestamp"])) / 1e3 / k
    print(f"queue {q}: {k} chains, period {period:.1f} us")
    print("   dur us  gap-before us  per chain  kernel")
    for name in order:
        print(f"{dur[name] / cnt[name]:9.1f} {gap[name] / cnt[name]:9.1f}      x{cnt[name] / k:4.2f}  "
              f"{name}")
    first = order[0]
    inner = sum(gap[n] for n in order) - gap[first]
    print(f"chain: kernels {kern / k:.1f} us, gaps inside {inner / k:.1f} us, first start to last "
          f"end {length / k:.1f} us, idle before the next chain {gap[first] / cnt[first]:.1f} us")


if __name__ == "__main__":
    main()
