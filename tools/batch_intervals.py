#!/usr/bin/env python3
"""Interval-overlap summary of the headline kernel's launches in a rocprofv3 --kernel-trace CSV.

    python tools/batch_intervals.py <run>_kernel_trace.csv [steps]     (steps: bench.py's --steps, default 20)

The timed region of `bench.py --steps S` is the last 4 S launches of k_spmv_blk; launch j of a step
belongs to matrix j (the sequence of handle j).  For each matrix's sequence: launches, mean duration,
mean gap to the previous launch of the same sequence, and how many of its launches intersect a launch
of each other sequence; plus queue / stream ids when the trace has them, and the region's span per launch.
Then what paces the region: per Queue_Id the sequences it carries, its busy time and share of the region, per
sequence the last end time, and the mean number of resident kernels (kernel time / span).
"""
import csv
import sys
from collections import defaultdict


def main():
    path = sys.argv[1]
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    batch = 4
    rows = [r for r in csv.DictReader(open(path)) if "k_spmv_blk" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    print(f"{len(rows)} k_spmv_blk launches in the trace; columns: {list(rows[0].keys())}")
    rows = rows[-batch * steps:]
    seqs = defaultdict(list)
    for i, r in enumerate(rows):
        seqs[i % batch].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r))
    t0 = min(s for q in seqs.values() for s, _, _ in q)
    t1 = max(e for q in seqs.values() for _, e, _ in q)
    n = sum(len(q) for q in seqs.values())
    print(f"timed region: {n} launches, span {(t1 - t0) / 1e3:.2f} us, span / launches {(t1 - t0) / 1e3 / n:.3f} us")
    for j in range(batch):
        q = seqs[j]
        dur = [e - s for s, e, _ in q]
        ids = {k: sorted({r.get(k, "") for _, _, r in q}) for k in ("Queue_Id", "Stream_Id") if k in q[0][2]}
        line = f"matrix {j}: {len(q)} launches, mean duration {sum(dur) / len(dur) / 1e3:.2f} us, ids {ids}"
        for k in range(batch):
            if k == j:
                continue
            hit = sum(1 for s, e, _ in q if any(s < e2 and s2 < e for s2, e2, _ in seqs[k]))
            line += f"; intersects seq {k}: {hit}/{len(q)}"
        print(line)
    # which queue paces the region: per Queue_Id the time a kernel of it is running (its own launches may
    # overlap, so the union), each sequence's last end, and the region's mean number of resident kernels
    span = t1 - t0
    if "Queue_Id" in rows[0]:
        byq = defaultdict(list)
        for j in range(batch):
            for s, e, r in seqs[j]:
                byq[r["Queue_Id"]].append((s, e, j))
        for qid in sorted(byq):
            busy, hi = 0, t0
            for s, e, _ in sorted(byq[qid]):
                busy += max(0, e - max(s, hi))
                hi = max(hi, e)
            carried = sorted({j for _, _, j in byq[qid]})
            print(f"queue {qid}: carries seq {carried}, {len(byq[qid])} launches, busy {busy / 1e3:.2f} us, "
                  f"{100.0 * busy / span:.1f} % of the region")
    ends = {j: max(e for _, e, _ in seqs[j]) for j in range(batch)}
    for j in range(batch):
        print(f"seq {j}: last end {(ends[j] - t0) / 1e3:.2f} us, {(t1 - ends[j]) / 1e3:.2f} us before the region's end")
    total = sum(e - s for q in seqs.values() for s, e, _ in q)
    print(f"mean resident kernels: {total / 1e3:.2f} us of kernel time / {span / 1e3:.2f} us span = {total / span:.2f}")
    # gaps between consecutive launches in dispatch order (the serial form: the launch boundary)
    allq = sorted((s, e) for q in seqs.values() for s, e, _ in q)
    gaps = [allq[i + 1][0] - allq[i][1] for i in range(len(allq) - 1)]
    print(f"start-ordered neighbours: mean gap {sum(gaps) / len(gaps) / 1e3:.3f} us, min {min(gaps) / 1e3:.3f}, "
          f"max {max(gaps) / 1e3:.3f} (negative = overlap)")
    print("first 12 launches of the region (start, end in us from region start):")
    for i, r in enumerate(rows[:12]):
        print(f"  seq {i % batch}: {(int(r['Start_Timestamp']) - t0) / 1e3:9.2f} {(int(r['End_Timestamp']) - t0) / 1e3:9.2f}")


if __name__ == "__main__":
    main()
