"""The crop box against the uncropped frame on one GPU: HIP-event march times (vr_timing_*) of C3 (MNI
stand-in, 1920 x 1080, 500 samples per ray), default and reset camera, exact and ESS | ERT, for
VR_MODE_DVR, VR_MODE_SDVR and VR_MODE_ISO under four settings of vr_set_crop_box:

  off     no box: the CROP = false instantiations, the parent's kernels
  whole   a box containing the volume: the same frame from the CROP = true instantiations -- their cost
  half    the half cut x < d_x / 2
  roi     a centred region of interest of a tenth of the volume (0.464 of every axis)

in one process and one context (the box is host state: setting it rebuilds nothing), the cases
alternating round by round after a warm-up, so drift of the box hits all of them alike.  Prints one JSON
document and writes it to --out.  --only off: the box-off cases alone (the A/B against another build of
the library, VR_LIB; profiles/crop/ab.txt).

    python tools/crop_probe.py --out profiles/crop/probe.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import volumerenderingproject_amd as vr  # noqa: E402
from volumerenderingproject_amd import volumes  # noqa: E402


def boxes(shape):
    d = [float(n) for n in shape]
    k = 0.1 ** (1.0 / 3.0)   # a tenth of the volume
    return {
        "off": None,
        "whole": ((-5.0, -5.0, -5.0), tuple(n + 5.0 for n in d)),
        "half": ((0.0, 0.0, 0.0), (0.5 * d[0], d[1], d[2])),
        "roi": (tuple(0.5 * n * (1.0 - k) for n in d), tuple(0.5 * n * (1.0 + k) for n in d)),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crop", "probe.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--frames", type=int, default=6, help="frames per case per round")
    ap.add_argument("--size", default="1920x1080x500")
    ap.add_argument("--only", default=None, help="one setting only (off: needs no vr_set_crop_box)")
    a = ap.parse_args()
    W, H, S = (int(v) for v in a.size.split("x"))
    vol, cal = volumes.mni152_standin()
    E, T = vr.VR_FLAG_ESS, vr.VR_FLAG_ERT
    modes = {"dvr": vr.VR_MODE_DVR, "sdvr": vr.VR_MODE_SDVR, "iso": vr.VR_MODE_ISO}
    cams = {"default": vr.default_camera(W, H), "reset": vr.reset_camera()}
    flags = {"exact": 0, "ess_ert": E | T}
    bx = boxes(vol.shape)
    settings = [a.only] if a.only else list(bx)
    r = vr.VolumeRenderer(vol, cal, device=0)
    frame = torch.empty((W, H, 4), dtype=torch.float32, device="cuda:0")
    cases = [(m, cam, fl, s) for m in modes for cam in cams for fl in flags for s in settings]

    def run(m, cam, fl, s, n):
        if not (a.only == "off"):
            if bx[s] is None:
                r.set_crop_box(None)
            else:
                r.set_crop_box(*bx[s])
        p = vr.default_params(W, H, S, mode=modes[m], flags=flags[fl])
        r.timing_read(reset=True)
        for _ in range(n):
            r.render_device(p, cams[cam], frame.data_ptr(), asynchronous=True)
        t = r.timing_read(reset=True)
        return t.total_ms / max(1, t.launches)

    r.timing_enable(True)
    for case in cases:   # warm-up: lazy state, work lists, caches, clocks
        run(*case, 2)
    samples = {case: [] for case in cases}
    for _ in range(a.rounds):
        for case in cases:
            samples[case].append(run(*case, a.frames))
    doc = {"source": "tools/crop_probe.py: HIP events around each march launch (vr_timing_read), ms per frame; "
                     "median and range over rounds, cases alternating in one process and one context",
           "device": torch.cuda.get_device_name(0), "volume": "MNI stand-in %dx%dx%d" % vol.shape, "frame": [W, H, S],
           "library": os.environ.get("VR_LIB", "in-tree"),
           "boxes": {k: v for k, v in bx.items() if k in settings},
           "rounds": a.rounds, "frames_per_round": a.frames, "results": []}
    for (m, cam, fl, s), v in samples.items():
        doc["results"].append({"mode": m, "camera": cam, "flags": fl, "box": s, "ms_median": round(statistics.median(v), 4),
                               "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)})
    med = {(x["mode"], x["camera"], x["flags"], x["box"]): x["ms_median"] for x in doc["results"]}
    if not a.only:
        for s in ("whole", "half", "roi"):   # time under the setting over the box-off time
            doc[f"{s}_over_off"] = {f"{m}/{cam}/{fl}": round(med[(m, cam, fl, s)] / med[(m, cam, fl, "off")], 3)
                                    for m in modes for cam in cams for fl in flags}
    r.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
