"""Timeline of the column path's two kernels from a rocprofv3 --kernel-trace CSV: the batched column
marches (vrc_march_kernel) and the expand passes (axis_expand_kernel) of vr_render_batch calls.

The dispatches are cut into calls in the order the host queued them (Dispatch_Id): a march launch adds
its frames (grid y) to the frames marched but not yet expanded, an expand takes one off, and a call
ends with the expand that brings the count to zero -- a pipelined call queues chunk k + 1's march
ahead of chunk k's expands, so inside a call the count stays positive.  Per call: the span of the
marches, the span of the expands, the time during which both kinds are running, and the expands' mean
duration with and without a march running beside them.  --show K also lists call K launch by launch with its stream (or
queue) id; the summary line is over the calls with --frames expands (the steady ones).

--fused: the trace of a library that renders the calls' frames with the fused column march
(vr_options.column_fused): no expand follows, so a call is the march launches whose frames add up to
--frames; per call its launches, their durations, the span and the time some launch is running.

usage: python tools/column_timeline.py <kernel_trace.csv> [--frames 32] [--show K] [--fused]"""
import argparse
import csv
import statistics


def union(iv):
    out = []
    for s, e in sorted(iv):
        if out and s <= out[-1][1]:
            out[-1][1] = max(out[-1][1], e)
        else:
            out.append([s, e])
    return out


def both(a, b):
    """Length of the intersection of two unions of intervals."""
    t = i = j = 0
    while i < len(a) and j < len(b):
        lo, hi = max(a[i][0], b[j][0]), min(a[i][1], b[j][1])
        t += max(0, hi - lo)
        if a[i][1] < b[j][1]:
            i += 1
        else:
            j += 1
    return t


def fused_calls(rows, a):
    calls, cur, n = [], [], 0
    for _, s, e, kind, where, frames in rows:
        if kind != "M":
            continue
        cur.append((s, e, where, frames))
        n += frames
        if n >= a.frames:
            if n == a.frames:
                calls.append(sorted(cur))
            cur, n = [], 0
    recs = []
    for k, call in enumerate(calls):
        t0, t1 = min(s for s, *_ in call), max(e for _, e, *_ in call)
        u = union([(s, e) for s, e, *_ in call])
        recs.append({"call": k, "launches": len(call), "span_us": (t1 - t0) / 1e3, "busy_us": sum(e - s for s, e in u) / 1e3,
                     "durations_us": "/".join(f"{(e - s) / 1e3:.1f}x{fr}" for s, e, _, fr in call)})
        if a.show == k:
            for s, e, where, fr in call:
                print(f"  F stream {where:>4}  frames {fr:3d}  start {(s - t0) / 1e3:8.2f} us  end {(e - t0) / 1e3:8.2f} us  "
                      f"dur {(e - s) / 1e3:6.2f} us")
        print(" ".join(f"{key}={v:.2f}" if isinstance(v, float) else f"{key}={v}" for key, v in recs[-1].items()))
    if recs:
        print(f"fused ({len(recs)} calls of {a.frames} frames), medians:")
        for key in ("launches", "span_us", "busy_us"):
            print(f"  {key} {statistics.median(r[key] for r in recs):.2f}")
        print(f"  span per frame {statistics.median(r['span_us'] for r in recs) / a.frames:.2f} us")
        gaps = [calls[i + 1][0][0] - max(e for _, e, *_ in calls[i]) for i in range(len(calls) - 1)]
        if gaps:
            print(f"  idle between calls {statistics.median(gaps) / 1e3:.2f} us")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("csv")
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--show", type=int, default=None)
    ap.add_argument("--fused", action="store_true")
    a = ap.parse_args()
    rows = []
    for r in csv.DictReader(open(a.csv)):
        kind = "M" if "vrc_march_kernel" in r["Kernel_Name"] else "E" if "axis_expand_kernel" in r["Kernel_Name"] else None
        if kind:
            where = r.get("Stream_Id") or r.get("Queue_Id") or "?"
            frames = int(r["Grid_Size_Y"]) // max(1, int(r["Workgroup_Size_Y"]))
            rows.append((int(r["Dispatch_Id"]), int(r["Start_Timestamp"]), int(r["End_Timestamp"]), kind, where, frames))
    rows.sort()
    if a.fused:
        fused_calls(rows, a)
        return
    calls, cur, pending = [], [], 0
    for _, s, e, kind, where, frames in rows:
        cur.append((s, e, kind, where))
        pending += frames if kind == "M" else -1
        if kind == "E" and pending <= 0:
            calls.append(sorted(cur))
            cur, pending = [], 0
    if cur:
        calls.append(sorted(cur))
    steady = []
    for k, call in enumerate(calls):
        m = [(s, e) for s, e, kind, _ in call if kind == "M"]
        x = [(s, e) for s, e, kind, _ in call if kind == "E"]
        if not m or not x:
            continue
        um, ux = union(m), union(x)
        t0, t1 = min(s for s, *_ in call), max(e for _, e, *_ in call)
        co = [e - s for s, e in x if both([[s, e]], um) > 0]
        alone = [e - s for s, e in x if both([[s, e]], um) == 0]
        rec = {"call": k, "marches": len(m), "expands": len(x), "span_us": (t1 - t0) / 1e3,
               "march_span_us": (um[-1][1] - um[0][0]) / 1e3, "march_busy_us": sum(e - s for s, e in um) / 1e3,
               "expand_span_us": (ux[-1][1] - ux[0][0]) / 1e3, "both_us": both(um, ux) / 1e3,
               "expand_mean_us": statistics.mean(e - s for s, e in x) / 1e3,
               "expand_with_march_us": statistics.mean(co) / 1e3 if co else None, "n_with_march": len(co),
               "expand_alone_us": statistics.mean(alone) / 1e3 if alone else None}
        if len(x) == a.frames:
            steady.append(rec)
        if a.show == k:
            for s, e, kind, where in call:
                print(f"  {kind} stream {where:>4}  start {(s - t0) / 1e3:8.2f} us  end {(e - t0) / 1e3:8.2f} us  "
                      f"dur {(e - s) / 1e3:6.2f} us")
        print(" ".join(f"{key}={v:.2f}" if isinstance(v, float) else f"{key}={v}" for key, v in rec.items()))
    if steady:
        print(f"steady ({len(steady)} calls of {a.frames} expands), medians:")
        for key in ("span_us", "march_span_us", "march_busy_us", "expand_span_us", "both_us", "expand_mean_us",
                    "expand_with_march_us", "expand_alone_us"):
            v = [r[key] for r in steady if r[key] is not None]
            print(f"  {key} {statistics.median(v):.2f}" if v else f"  {key} none")
        print(f"  span per frame {statistics.median(r['span_us'] for r in steady) / a.frames:.2f} us")


if __name__ == "__main__":
    main()
