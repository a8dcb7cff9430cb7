"""SDVR against DVR on one GPU: HIP-event march times (vr_timing_*) of C3 (MNI stand-in, 1920 x 1080,
500 samples per ray), default and reset camera, exact and ESS | ERT, for

  dvr_byte    VR_MODE_DVR from the byte copy of the volume -- the yardstick (profiles/dvr/probe.json's
              configuration, re-taken here)
  sdvr_byte   VR_MODE_SDVR from the byte copy: per shaded sample six more taps of four dword gathers
  sdvr_float  VR_MODE_SDVR from the float volume (vr_options.dvr_volume = 1): eight float gathers per tap

the two SDVR configurations under the coefficient sets SH_KS0 (0.3, 0.7, 0, 16) and SH_GEN
(0.3, 0.7, 0.2, 16), in one process, the configurations alternating round by round after a warm-up, so
drift of the box hits all of them alike.  Prints one JSON document and writes it to --out.

    python tools/sdvr_probe.py --out profiles/sdvr/probe.json
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

SHADE = {"ks0": (0.3, 0.7, 0.0, 16.0), "gen": (0.3, 0.7, 0.2, 16.0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sdvr", "probe.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--frames", type=int, default=10, help="frames per configuration per round")
    ap.add_argument("--size", default="1920x1080x500")
    a = ap.parse_args()
    W, H, S = (int(v) for v in a.size.split("x"))
    vol, cal = volumes.mni152_standin()
    E, T = vr.VR_FLAG_ESS, vr.VR_FLAG_ERT
    # configuration -> (context, mode, coefficient set)
    configs = {"dvr_byte": ("byte", vr.VR_MODE_DVR, None)}
    for s in SHADE:
        configs[f"sdvr_byte/{s}"] = ("byte", vr.VR_MODE_SDVR, s)
        configs[f"sdvr_float/{s}"] = ("float", vr.VR_MODE_SDVR, s)
    ctx = {"byte": vr.VolumeRenderer(vol, cal, device=0),
           "float": vr.VolumeRenderer(vol, cal, device=0, options=vr.default_options(dvr_volume=1))}
    cams = {"default": vr.default_camera(W, H), "reset": vr.reset_camera()}
    flags = {"exact": 0, "ess_ert": E | T}
    frame = torch.empty((W, H, 4), dtype=torch.float32, device="cuda:0")
    cases = [(c, cam, fl) for c in configs for cam in cams for fl in flags]

    def run(c, cam, fl, n):
        which, mode, shade = configs[c]
        r = ctx[which]
        p = vr.default_params(W, H, S, mode=mode, flags=flags[fl])
        if shade is not None:
            p.shade_ambient, p.shade_diffuse, p.shade_specular, p.shade_shininess = SHADE[shade]
        r.timing_read(reset=True)
        for _ in range(n):
            r.render_device(p, cams[cam], frame.data_ptr(), asynchronous=True)
        t = r.timing_read(reset=True)
        return t.total_ms / max(1, t.launches)

    for r in ctx.values():
        r.timing_enable(True)
    for case in cases:   # warm-up: lazy state, work lists, caches, clocks
        run(*case, 3)
    samples = {case: [] for case in cases}
    for _ in range(a.rounds):
        for case in cases:
            samples[case].append(run(*case, a.frames))
    doc = {"source": "tools/sdvr_probe.py: HIP events around each march launch (vr_timing_read), ms per frame; "
                     "median and range over rounds, configurations alternating in one process",
           "device": torch.cuda.get_device_name(0), "volume": "MNI stand-in 182x218x182", "frame": [W, H, S],
           "rounds": a.rounds, "frames_per_round": a.frames, "shade": SHADE, "results": []}
    med = {case: statistics.median(v) for case, v in samples.items()}
    for (c, cam, fl), v in samples.items():
        doc["results"].append({"config": c, "camera": cam, "flags": fl, "ms_median": round(med[(c, cam, fl)], 4),
                               "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
                               "over_dvr_byte": round(med[(c, cam, fl)] / med[("dvr_byte", cam, fl)], 3)})
    for r in ctx.values():
        r.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
