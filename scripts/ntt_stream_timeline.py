#!/usr/bin/env python3
"""Per-step stream timeline of the two-stream batched Goldilocks NTT (ntt_launch.hip
run_gl_passes), from a `rocprofv3 --kernel-trace` csv (a kernel trace in a run of its own, no
counters alongside) of any program that runs warm-up steps of one batched transform, leaves the
GPU idle for at least 3 ms, then runs the timed steps back to back: the kernels whose names
contain "ntt" after the last such gap are the timed ones.

  python scripts/ntt_stream_timeline.py <kernel_trace.csv> <steps>

The timed kernels are cut into `steps` equal runs in start order (every step launches the same
kernels). The caller's stream is the queue whose kernel opens most steps and the auxiliary
stream is the other queue. Per step and as medians over the steps, in microseconds:
  (a) fork lag: the auxiliary stream's first kernel start minus the caller stream's first start;
  (b) alone time at the end: each stream's last kernel end to the other stream's last kernel end
      (aux_tail > 0: the auxiliary stream finishes last and the caller's stream waits for it);
  (c) step gap: the step's last kernel end to the next step's first kernel start (the join's
      latency plus the next call's fork record);
  (d) the kernel-union busy time against the window (first start .. next step's first start; for
      the last step .. its last end).
"""
import csv
import statistics
import sys


def timed_kernels(path):
    """(start, end, queue) of the NTT kernels after the last >= 3 ms idle gap, in start order."""
    rows = [r for r in csv.DictReader(open(path)) if "ntt" in r["Kernel_Name"]]
    ev = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Queue_Id"]) for r in rows)
    cut = 0
    for i in range(1, len(ev)):
        if ev[i][0] - max(e for _, e, _ in ev[max(0, i - 64):i]) > 3_000_000:  # ns
            cut = i
    return ev[cut:], cut


def union_busy(kernels):
    busy, cur_s, cur_e = 0, None, None
    for s, e, _ in kernels:
        if cur_e is None or s > cur_e:
            if cur_e is not None:
                busy += cur_e - cur_s
            cur_s, cur_e = s, e
        else:
            cur_e = max(cur_e, e)
    return busy + (cur_e - cur_s)


def decompose(timed, steps):
    if len(timed) % steps:
        raise SystemExit(f"{len(timed)} timed kernels do not divide into {steps} steps")
    per = len(timed) // steps
    firsts = [timed[k * per][2] for k in range(steps)]
    caller = max(set(firsts), key=firsts.count)  # the queue that opens most steps
    out = []
    for k in range(steps):
        ks = timed[k * per:(k + 1) * per]
        mine = [x for x in ks if x[2] == caller]
        aux = [x for x in ks if x[2] != caller]
        first, last = ks[0][0], max(e for _, e, _ in ks)
        nxt = timed[(k + 1) * per][0] if k + 1 < steps else None
        row = {"kernels": per, "streams": len({q for _, _, q in ks}),
               "busy": union_busy(ks) / 1e3, "window": ((nxt if nxt is not None else last) - first) / 1e3,
               "gap": (nxt - last) / 1e3 if nxt is not None else None}
        if aux:
            row["fork_lag"] = (aux[0][0] - mine[0][0]) / 1e3
            row["aux_tail"] = (max(e for _, e, _ in aux) - max(e for _, e, _ in mine)) / 1e3
        out.append(row)
    return out


def main():
    path, steps = sys.argv[1], int(sys.argv[2])
    timed, cut = timed_kernels(path)
    rows = decompose(timed, steps)
    print(f"timed kernels: {len(timed)} over {steps} steps, {rows[0]['kernels']} per step on "
          f"{rows[0]['streams']} queue(s) (warm-up kernels before the idle gap: {cut})")
    print("step  (a) fork_lag  (b) aux_tail  (c) gap_to_next  (d) busy / window   [us; aux_tail > 0: the "
          "auxiliary stream ends last]")

    def f(v):
        return "       -" if v is None else f"{v:8.1f}"

    for k, r in enumerate(rows):
        print(f"{k:4d}  {f(r.get('fork_lag'))}      {f(r.get('aux_tail'))}      {f(r['gap'])}         "
              f"{r['busy']:7.1f} / {r['window']:7.1f}")

    def med(key, rs=rows):
        v = [r[key] for r in rs if r.get(key) is not None]
        return statistics.median(v) if v else None

    full = rows[:-1] if steps > 1 else rows  # steps whose window ends at the next step's first kernel
    busy, window = med("busy", full), med("window", full)
    print(f"median (a) fork lag {f(med('fork_lag'))} us   (b) aux tail {f(med('aux_tail'))} us   "
          f"(c) gap to next step {f(med('gap'))} us")
    print(f"median (d) kernel-union busy {busy:.1f} us of a {window:.1f}-us window per step "
          f"(idle {window - busy:.1f} us, {100 * (window - busy) / window:.1f} %)")
    span = (max(e for _, e, _ in timed) - timed[0][0]) / 1e3
    print(f"whole timed region: busy {sum(r['busy'] for r in rows) / steps:.1f} us, window {span / steps:.1f} us "
          f"per step (first start .. last end over {steps} steps)")


if __name__ == "__main__":
    main()
