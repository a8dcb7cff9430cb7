"""SCDVR against SDVR and CDVR on one GPU: HIP-event march times (vr_timing_*) of C3 (MNI stand-in,
1920 x 1080, 500 samples per ray), default and reset (oblique) camera, the four flag combinations, for

  cdvr_byte / cdvr_float     VR_MODE_CDVR under the skin-to-bone ramp -- the yardstick of the classification
  sdvr_byte / sdvr_float     VR_MODE_SDVR under the default interval TF -- the yardstick of the lighting
  scdvr_byte / scdvr_float   VR_MODE_SCDVR under the same ramp, with G = unit (the context's first map) and
                             with G = edges (flat tissue transparent, a ramp to full weight at boundaries)

from the byte copy of the volume and from the float volume (vr_options.dvr_volume = 1), in one process, one
context per volume kind, the configurations alternating round by round after a warm-up, so drift of the
box hits all of them alike.  The coefficients are SH_KS0 (0.3, 0.7, 0, 16) throughout.  G travels with each
launch, so switching it costs nothing.  Prints one JSON document and writes it to --out.

    python tools/scdvr_probe.py --out profiles/scdvr/probe.json
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

SKIN_BONE = [(0.0, (0.0, 0.0, 0.0, 0.0)), (40.0, (0.0, 0.0, 0.0, 0.0)), (90.0, (0.85, 0.55, 0.45, 0.03)),
             (150.0, (0.9, 0.7, 0.6, 0.08)), (200.0, (1.0, 0.95, 0.85, 0.5)), (255.0, (1.0, 1.0, 1.0, 0.9))]
GOPAS = {"unit": [(0.0, 1.0)], "edges": [(1.5, 0.0), (8.0, 0.25), (80.0, 1.0)]}
SH_KS0 = (0.3, 0.7, 0.0, 16.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scdvr", "probe.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--frames", type=int, default=20, help="frames per configuration per round")
    ap.add_argument("--size", default="1920x1080x500")
    a = ap.parse_args()
    W, H, S = (int(v) for v in a.size.split("x"))
    vol, cal = volumes.mni152_standin()
    E, T = vr.VR_FLAG_ESS, vr.VR_FLAG_ERT
    # configuration -> (context, mode, G)
    configs = {}
    for kind in ("byte", "float"):
        configs[f"cdvr_{kind}"] = (kind, vr.VR_MODE_CDVR, None)
        configs[f"sdvr_{kind}"] = (kind, vr.VR_MODE_SDVR, None)
        for g in GOPAS:
            configs[f"scdvr_{kind}/{g}"] = (kind, vr.VR_MODE_SCDVR, g)
    ctx = {"byte": vr.VolumeRenderer(vol, cal, device=0),
           "float": vr.VolumeRenderer(vol, cal, device=0, options=vr.default_options(dvr_volume=1))}
    for r in ctx.values():
        r.set_colormap(SKIN_BONE)
    cams = {"default": vr.default_camera(W, H), "reset": vr.reset_camera()}
    flags = {"exact": 0, "ess": E, "ert": T, "ess_ert": E | T}
    frame = torch.empty((W, H, 4), dtype=torch.float32, device="cuda:0")
    cases = [(c, cam, fl) for c in configs for cam in cams for fl in flags]

    def run(c, cam, fl, n):
        which, mode, g = configs[c]
        r = ctx[which]
        if g is not None:
            r.set_gradient_opacity(GOPAS[g])
        p = vr.default_params(W, H, S, mode=mode, flags=flags[fl])
        p.shade_ambient, p.shade_diffuse, p.shade_specular, p.shade_shininess = SH_KS0
        r.timing_read(reset=True)
        for _ in range(n):
            r.render_device(p, cams[cam], frame.data_ptr(), asynchronous=True)
        t = r.timing_read(reset=True)
        return t.total_ms / max(1, t.launches)

    for r in ctx.values():
        r.timing_enable(True)
    for case in cases:   # warm-up: lazy state, work lists, caches, clocks
        run(*case, 2)
    samples = {case: [] for case in cases}
    for _ in range(a.rounds):
        for case in cases:
            samples[case].append(run(*case, a.frames))
    doc = {"source": "tools/scdvr_probe.py: HIP events around each march launch (vr_timing_read), ms per frame; "
                     "median and range over rounds, configurations alternating in one process",
           "device": torch.cuda.get_device_name(0), "volume": "MNI stand-in 182x218x182", "frame": [W, H, S],
           "rounds": a.rounds, "frames_per_round": a.frames, "colormap": SKIN_BONE, "gradient_opacity": GOPAS,
           "shade": SH_KS0, "results": []}
    med = {case: statistics.median(v) for case, v in samples.items()}
    for (c, cam, fl), v in samples.items():
        kind = "float" if "float" in c else "byte"
        doc["results"].append({"config": c, "camera": cam, "flags": fl, "ms_median": round(med[(c, cam, fl)], 4),
                               "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
                               "over_cdvr": round(med[(c, cam, fl)] / med[(f"cdvr_{kind}", cam, fl)], 3),
                               "over_sdvr": round(med[(c, cam, fl)] / med[(f"sdvr_{kind}", cam, fl)], 3)})
    for r in ctx.values():
        r.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
