"""Device-only time per frame of C3 vr_render_batch calls: eight 32-frame calls are queued while the
stream is held busy (torch.cuda._sleep), so the host is out of the timed window (events on the caller's
stream either side of the calls).  Prints one JSON line: per vr_options.column_overlap value (-1 = the
library's default; the only value a library without the option takes) the min, median and max of seven
repetitions, in us per frame.  A second list gives vr_options.column_fused values (keys "overlap/fused").

usage: python tools/device_only_time.py 0,1 [0,1]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch
    import volumerenderingproject_amd as vr
    from volumerenderingproject_amd import volumes
    vals = [(int(x), None) for x in sys.argv[1].split(",")]
    if len(sys.argv) > 2:
        vals = [(ov, int(fv)) for ov, _ in vals for fv in sys.argv[2].split(",")]
    vol, cal = volumes.mni152_standin()
    W, H, S = 1920, 1080, 500
    n, calls = 32, 8
    p = vr.default_params(W, H, S, flags=vr.VR_FLAG_ESS | vr.VR_FLAG_ERT)
    frames = torch.empty((n, W, H, 4), dtype=torch.float32, device="cuda:0")
    cams = (vr.Camera * n)(*([vr.default_camera(W, H)] * n))
    out = {}
    for ov, fv in vals:
        o = vr.default_options()
        if ov >= 0:
            o.column_overlap = ov
        if fv is not None:
            o.column_fused = fv
        r = vr.VolumeRenderer(vol, cal, device=0, options=o)
        stream = torch.cuda.Stream(device=0)
        torch.cuda.set_stream(stream)
        r.set_stream(stream.cuda_stream)
        for _ in range(3):
            r.render_batch_device(p, cams, frames.data_ptr())
        torch.cuda.synchronize()
        res = []
        for _ in range(7):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda._sleep(60_000_000)
            e0.record(stream)
            for _ in range(calls):
                r.render_batch_device(p, cams, frames.data_ptr(), asynchronous=True)
            e1.record(stream)
            torch.cuda.synchronize()
            res.append(e0.elapsed_time(e1) * 1e3 / (n * calls))
        res.sort()
        out[str(ov) if fv is None else f"{ov}/{fv}"] = {"min": round(res[0], 3), "median": round(res[len(res) // 2], 3), "max": round(res[-1], 3)}
        r.set_stream(0)
        r.close()
    print(json.dumps({"device_us_per_frame": out, "lib": os.path.basename(os.environ.get("VR_LIB") or "libvr.so")}))


if __name__ == "__main__":
    main()
