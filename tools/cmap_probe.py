"""CDVR against DVR on one GPU: HIP-event march times (vr_timing_*) of C3 (MNI stand-in, 1920 x 1080,
500 samples per ray), default and reset camera, exact and ESS | ERT, for

  dvr_byte / dvr_float     VR_MODE_DVR under the default interval TF -- the yardsticks
  cdvr_byte / cdvr_float   VR_MODE_CDVR from the byte copy of the volume and from the float volume
                           (vr_options.dvr_volume = 1), under a 5-point map (the sum of compares over
                           wave-uniform x) and under a 256-point map (the LDS binary search)

in one process, one context per volume kind, the configurations alternating round by round after a
warm-up, so drift of the box hits all of them alike.  Both maps are transparent at 0 and over the air, like
the default TF.  Prints one JSON document and writes it to --out.

    python tools/cmap_probe.py --out profiles/cmap/probe.json
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

MAP5 = [(0.0, (0.0, 0.0, 0.0, 0.0)), (40.0, (0.0, 0.0, 0.0, 0.0)), (90.0, (0.85, 0.55, 0.45, 0.03)),
        (180.0, (1.0, 0.9, 0.8, 0.3)), (255.0, (1.0, 1.0, 1.0, 0.9))]


def map256():
    """MAP5 resampled at 256 points: the same function, through the other search."""
    return [(float(i), tuple(float(c) for c in vr.colormap_eval(MAP5, [float(i)])[0])) for i in range(256)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cmap", "probe.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--frames", type=int, default=10, help="frames per configuration per round")
    ap.add_argument("--size", default="1920x1080x500")
    a = ap.parse_args()
    W, H, S = (int(v) for v in a.size.split("x"))
    vol, cal = volumes.mni152_standin()
    E, T = vr.VR_FLAG_ESS, vr.VR_FLAG_ERT
    maps = {"map5": MAP5, "map256": map256()}
    assert len(maps["map256"]) == 256
    # configuration -> (context, mode, map)
    configs = {}
    for kind in ("byte", "float"):
        configs[f"dvr_{kind}"] = (kind, vr.VR_MODE_DVR, None)
        for m in maps:
            configs[f"cdvr_{kind}/{m}"] = (kind, vr.VR_MODE_CDVR, m)
    ctx = {"byte": vr.VolumeRenderer(vol, cal, device=0),
           "float": vr.VolumeRenderer(vol, cal, device=0, options=vr.default_options(dvr_volume=1))}
    current = {k: None for k in ctx}
    cams = {"default": vr.default_camera(W, H), "reset": vr.reset_camera()}
    flags = {"exact": 0, "ess_ert": E | T}
    frame = torch.empty((W, H, 4), dtype=torch.float32, device="cuda:0")
    cases = [(c, cam, fl) for c in configs for cam in cams for fl in flags]

    def run(c, cam, fl, n):
        which, mode, m = configs[c]
        r = ctx[which]
        if m is not None and current[which] != m:   # (the tables are rebuilt by the first frame below)
            r.set_colormap(maps[m])
            current[which] = m
            r.render_device(vr.default_params(W, H, S, mode=mode, flags=flags[fl]), cams[cam], frame.data_ptr())
        p = vr.default_params(W, H, S, mode=mode, flags=flags[fl])
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
    doc = {"source": "tools/cmap_probe.py: HIP events around each march launch (vr_timing_read), ms per frame; "
                     "median and range over rounds, configurations alternating in one process",
           "device": torch.cuda.get_device_name(0), "volume": "MNI stand-in 182x218x182", "frame": [W, H, S],
           "rounds": a.rounds, "frames_per_round": a.frames, "map5": MAP5, "results": []}
    med = {case: statistics.median(v) for case, v in samples.items()}
    for (c, cam, fl), v in samples.items():
        yard = "dvr_float" if "float" in c else "dvr_byte"
        doc["results"].append({"config": c, "camera": cam, "flags": fl, "ms_median": round(med[(c, cam, fl)], 4),
                               "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
                               "over_dvr": round(med[(c, cam, fl)] / med[(yard, cam, fl)], 3)})
    for r in ctx.values():
        r.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
