"""DVR against its yardstick on one GPU: HIP-event march times (vr_timing_*) of C3 (MNI stand-in,
1920 x 1080, 500 samples per ray), default and reset camera, exact and ESS | ERT, for

  dvr_byte    VR_MODE_DVR, four dword gathers per sample from the byte copy of the volume
  dvr_float   VR_MODE_DVR, eight float gathers (vr_options.dvr_volume = 1)
  test        VR_MODE_TEST at its defaults (corner volume, plane table; the axis kernel on the default view)
  test_rows   VR_MODE_TEST with test_corners = 2: the same positions and the same four dword gathers
              per sample as dvr_byte -- the yardstick
  test_rows_general  the same with test_plane_march = 0: the general march on the default view too
              (there TEST otherwise takes its axis kernel, which DVR has no counterpart of yet)

in one process, the configurations alternating round by round after a warm-up, so drift of the box
hits all of them alike.  Prints one JSON document and writes it to --out.

    python tools/dvr_probe.py --out profiles/dvr/probe.json
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dvr", "probe.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--frames", type=int, default=10, help="frames per configuration per round")
    ap.add_argument("--size", default="1920x1080x500")
    a = ap.parse_args()
    W, H, S = (int(v) for v in a.size.split("x"))
    vol, cal = volumes.mni152_standin()
    E, T = vr.VR_FLAG_ESS, vr.VR_FLAG_ERT
    configs = {
        "dvr_byte": (vr.VR_MODE_DVR, {}),
        "dvr_float": (vr.VR_MODE_DVR, {"dvr_volume": 1}),
        "test": (vr.VR_MODE_TEST, {}),
        "test_rows": (vr.VR_MODE_TEST, {"test_corners": 2}),
        "test_rows_general": (vr.VR_MODE_TEST, {"test_corners": 2, "test_plane_march": 0}),
    }
    ctx = {k: vr.VolumeRenderer(vol, cal, device=0, options=vr.default_options(**o)) for k, (_, o) in configs.items()}
    cams = {"default": vr.default_camera(W, H), "reset": vr.reset_camera()}
    flags = {"exact": 0, "ess_ert": E | T}
    frame = torch.empty((W, H, 4), dtype=torch.float32, device="cuda:0")
    cases = [(c, cam, fl) for c in configs for cam in cams for fl in flags]

    def run(c, cam, fl, n):
        r = ctx[c]
        p = vr.default_params(W, H, S, mode=configs[c][0], flags=flags[fl])
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
    doc = {"source": "tools/dvr_probe.py: HIP events around each march launch (vr_timing_read), ms per frame; "
                     "median and range over rounds, configurations alternating in one process",
           "device": torch.cuda.get_device_name(0), "volume": "MNI stand-in 182x218x182", "frame": [W, H, S],
           "rounds": a.rounds, "frames_per_round": a.frames, "results": []}
    for (c, cam, fl), v in samples.items():
        doc["results"].append({"config": c, "camera": cam, "flags": fl, "ms_median": round(statistics.median(v), 4),
                               "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)})
    med = {(r["config"], r["camera"], r["flags"]): r["ms_median"] for r in doc["results"]}
    for y in ("test_rows", "test_rows_general"):
        doc[f"dvr_byte_over_{y}"] = {f"{cam}/{fl}": round(med[("dvr_byte", cam, fl)] / med[(y, cam, fl)], 3)
                                     for cam in cams for fl in flags}
    for r in ctx.values():
        r.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
