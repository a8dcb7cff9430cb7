"""VR_FLAG_PERSP against the orthographic frame on one GPU: HIP-event march times (vr_timing_*) of C3 (MNI
stand-in, 1920 x 1080, 500 samples per ray), default and reset (oblique) camera direction, exact and
ESS | ERT, for VR_MODE_DVR, VR_MODE_SDVR and VR_MODE_ISO:

  ortho   the frame without the flag: the parent's kernels, the default screen and the cameras of bench.py
  persp   the flag, the screen from vr_persp_screen at --fov degrees (default 54) and the default viewplane
          distance, the eye on the orthographic camera's line of sight at the distance D from the volume's
          centre at which the frustum's cross-section is the orthographic screen: D = rsh_ortho / (2 tan(fov / 2))
          (1.104 at 54 degrees: the whole volume lies between the eye and sample S, and the samples of the
          centre ray are spaced as the orthographic ones, vpd / S)

in one process and one context, the cases alternating round by round after a warm-up, so drift of the machine
hits all of them alike.  The share of drawing pixels (pixels off the background) of both frames is recorded
beside the times: it says how comparable the two frames' work is.  Prints one JSON document and writes it to
--out.

    python tools/persp_probe.py --out profiles/persp/probe.json
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import volumerenderingproject_amd as vr  # noqa: E402
from volumerenderingproject_amd import volumes  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "persp", "probe.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--frames", type=int, default=6, help="frames per case per round")
    ap.add_argument("--size", default="1920x1080x500")
    ap.add_argument("--fov", type=float, default=54.0, help="vertical field of view of the perspective frames, degrees")
    a = ap.parse_args()
    W, H, S = (int(v) for v in a.size.split("x"))
    vol, cal = volumes.mni152_standin()
    E, T = vr.VR_FLAG_ESS, vr.VR_FLAG_ERT
    modes = {"dvr": vr.VR_MODE_DVR, "sdvr": vr.VR_MODE_SDVR, "iso": vr.VR_MODE_ISO}
    flags = {"exact": 0, "ess_ert": E | T}
    base = vr.default_params(W, H, S)
    rsw, rsh = vr.persp_screen(a.fov, W, H, base.viewplane_distance)
    dist = base.real_screen_height / (2.0 * math.tan(math.radians(a.fov) / 2.0))
    ortho_cams = {"default": vr.default_camera(W, H), "reset": vr.reset_camera()}
    persp_cams = {}
    for name, c in ortho_cams.items():
        n = math.sqrt(sum(float(v) ** 2 for v in c.pos))
        persp_cams[name] = vr.derive_camera(tuple(float(v) / n * dist for v in c.pos), tuple(c.up), rsw, rsh)

    def params(m, fl, proj):
        p = vr.default_params(W, H, S, mode=modes[m], flags=flags[fl] | (vr.VR_FLAG_PERSP if proj == "persp" else 0))
        if proj == "persp":
            p.real_screen_width, p.real_screen_height = rsw, rsh
        return p

    def camera(cam, proj):
        return (persp_cams if proj == "persp" else ortho_cams)[cam]

    r = vr.VolumeRenderer(vol, cal, device=0)
    frame = torch.empty((W, H, 4), dtype=torch.float32, device="cuda:0")
    cases = [(m, cam, fl, proj) for m in modes for cam in ortho_cams for fl in flags for proj in ("ortho", "persp")]

    def run(m, cam, fl, proj, n):
        p = params(m, fl, proj)
        r.timing_read(reset=True)
        for _ in range(n):
            r.render_device(p, camera(cam, proj), frame.data_ptr(), asynchronous=True)
        t = r.timing_read(reset=True)
        return t.total_ms / max(1, t.launches)

    # the share of drawing pixels, from the exact frames
    bg = np.array(list(base.background), np.float32)[:3]
    share = {}
    for m in modes:
        for cam in ortho_cams:
            for proj in ("ortho", "persp"):
                f = r.render(params(m, "exact", proj), camera(cam, proj))
                share[(m, cam, proj)] = float(np.any(f[..., :3] != bg, axis=-1).mean())
    r.timing_enable(True)
    for case in cases:   # warm-up: lazy state, work lists, caches, clocks
        run(*case, 2)
    samples = {case: [] for case in cases}
    for _ in range(a.rounds):
        for case in cases:
            samples[case].append(run(*case, a.frames))
    doc = {"source": "tools/persp_probe.py: HIP events around each march launch (vr_timing_read), ms per frame; "
                     "median and range over rounds, cases alternating in one process and one context",
           "device": torch.cuda.get_device_name(0), "volume": "MNI stand-in %dx%dx%d" % vol.shape, "frame": [W, H, S],
           "fov_y_degrees": a.fov, "persp_screen": [rsw, rsh], "persp_eye_distance": round(dist, 4),
           "ortho_screen": [base.real_screen_width, base.real_screen_height],
           "viewplane_distance": base.viewplane_distance,
           "rounds": a.rounds, "frames_per_round": a.frames, "results": []}
    for (m, cam, fl, proj), v in samples.items():
        doc["results"].append({"mode": m, "camera": cam, "flags": fl, "projection": proj,
                               "ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4),
                               "ms_max": round(max(v), 4), "drawing_share": round(share[(m, cam, proj)], 4)})
    med = {(x["mode"], x["camera"], x["flags"], x["projection"]): x["ms_median"] for x in doc["results"]}
    doc["persp_over_ortho"] = {f"{m}/{cam}/{fl}": round(med[(m, cam, fl, "persp")] / med[(m, cam, fl, "ortho")], 3)
                               for m in modes for cam in ortho_cams for fl in flags}
    r.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
