"""MIP against its yardstick on one GPU: HIP-event march times (vr_timing_*) of C3 (MNI stand-in,
1920 x 1080, 500 samples per ray), default and reset camera, for

  mip            VR_MODE_MIP without flags: every in-volume sample of every ray
  mip_ess        VR_MODE_MIP, VR_FLAG_ESS: a ray skips the cells that cannot raise its maximum
  mip_ess_ert    VR_MODE_MIP, VR_FLAG_ESS | VR_FLAG_ERT: and stops at the volume-wide bound
  dvr            VR_MODE_DVR exact -- the yardstick: the same positions and gathers, plus the
                 classification and the blend
  dvr_ess_ert    VR_MODE_DVR, VR_FLAG_ESS | VR_FLAG_ERT

in one process and on one context (both modes share the byte copy of the volume), the configurations
alternating round by round after a warm-up, so drift of the box hits all of them alike.  Checks once
that the three MIP frames of a camera are equal, prints one JSON document and writes it to --out.

    python tools/mip_probe.py --out profiles/mip/probe.json
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mip", "probe.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--frames", type=int, default=10, help="frames per configuration per round")
    ap.add_argument("--size", default="1920x1080x500")
    a = ap.parse_args()
    W, H, S = (int(v) for v in a.size.split("x"))
    vol, cal = volumes.mni152_standin()
    E, T = vr.VR_FLAG_ESS, vr.VR_FLAG_ERT
    configs = {
        "mip": (vr.VR_MODE_MIP, 0),
        "mip_ess": (vr.VR_MODE_MIP, E),
        "mip_ess_ert": (vr.VR_MODE_MIP, E | T),
        "dvr": (vr.VR_MODE_DVR, 0),
        "dvr_ess_ert": (vr.VR_MODE_DVR, E | T),
    }
    r = vr.VolumeRenderer(vol, cal, device=0)
    cams = {"default": vr.default_camera(W, H), "reset": vr.reset_camera()}
    frame = torch.empty((W, H, 4), dtype=torch.float32, device="cuda:0")
    cases = [(c, cam) for c in configs for cam in cams]

    def run(c, cam, n):
        mode, flags = configs[c]
        p = vr.default_params(W, H, S, mode=mode, flags=flags)
        r.timing_read(reset=True)
        for _ in range(n):
            r.render_device(p, cams[cam], frame.data_ptr(), asynchronous=True)
        t = r.timing_read(reset=True)
        return t.total_ms / max(1, t.launches)

    r.timing_enable(True)
    same = {}
    for cam in cams:   # warm-up (lazy state, work lists, caches, clocks), and the frames compared once
        kept = None
        for c in configs:
            run(c, cam, 3)
            if configs[c][0] == vr.VR_MODE_MIP:
                r.synchronize()
                if kept is None:
                    kept = frame.clone()
                same[f"{cam}/{c}"] = bool(torch.equal(frame, kept))
    samples = {case: [] for case in cases}
    for _ in range(a.rounds):
        for case in cases:
            samples[case].append(run(*case, a.frames))
    doc = {"source": "tools/mip_probe.py: HIP events around each march launch (vr_timing_read), ms per frame; "
                     "median and range over rounds, configurations alternating in one process",
           "device": torch.cuda.get_device_name(0), "volume": "MNI stand-in 182x218x182", "frame": [W, H, S],
           "rounds": a.rounds, "frames_per_round": a.frames, "mip_frames_equal": same, "results": []}
    for (c, cam), v in samples.items():
        doc["results"].append({"config": c, "camera": cam, "ms_median": round(statistics.median(v), 4),
                               "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)})
    med = {(x["config"], x["camera"]): x["ms_median"] for x in doc["results"]}
    doc["mip_over_dvr_exact"] = {cam: round(med[("mip", cam)] / med[("dvr", cam)], 3) for cam in cams}
    doc["mip_ess_over_mip"] = {cam: round(med[("mip_ess", cam)] / med[("mip", cam)], 3) for cam in cams}
    doc["mip_ess_ert_over_mip_ess"] = {cam: round(med[("mip_ess_ert", cam)] / med[("mip_ess", cam)], 3) for cam in cams}
    r.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
