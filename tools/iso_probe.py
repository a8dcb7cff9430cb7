"""ISO against its yardstick on one GPU: HIP-event march times (vr_timing_*) of C3 (MNI stand-in,
1920 x 1080, 500 samples per ray, isovalue = half of cal_max), default and reset (oblique) camera, for

  iso            VR_MODE_ISO without flags: every in-volume sample of a ray up to its hit
  iso_ess_ert    VR_MODE_ISO, VR_FLAG_ESS | VR_FLAG_ERT: a ray skips the cells bounded below the isovalue
  mip_ess        VR_MODE_MIP, VR_FLAG_ESS -- the yardstick: the same positions, gathers and cell bounds,
                 pruned against a running maximum, every ray marched to its exit

in one process and on one context (both modes share the byte copy of the volume and the cell bounds),
the configurations alternating round by round after the same warm-up, so drift of the box hits all of
them alike.  Checks once that the two ISO frames of a camera are equal.  The condition recorded: the
iso_ess_ert median does not exceed the mip_ess median by more than the run-to-run spread (max - min
over the rounds) of the mip_ess figure.  Prints one JSON document and writes it to --out.

    python tools/iso_probe.py --out profiles/iso/probe.json
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "iso", "probe.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--frames", type=int, default=10, help="frames per configuration per round")
    ap.add_argument("--size", default="1920x1080x500")
    a = ap.parse_args()
    W, H, S = (int(v) for v in a.size.split("x"))
    vol, cal = volumes.mni152_standin()
    E, T = vr.VR_FLAG_ESS, vr.VR_FLAG_ERT
    configs = {
        "iso": (vr.VR_MODE_ISO, 0),
        "iso_ess_ert": (vr.VR_MODE_ISO, E | T),
        "mip_ess": (vr.VR_MODE_MIP, E),
    }
    r = vr.VolumeRenderer(vol, cal, device=0)
    iso_value, rgb = r.isosurface   # (a context starts at half of cal_max, white)
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
    same, hit_fraction = {}, {}
    bg = torch.tensor(list(vr.default_params(W, H, S).background)[:3], device="cuda:0")
    for cam in cams:   # warm-up (lazy state, work lists, caches, clocks), and the frames compared once
        kept = None
        for c in configs:
            run(c, cam, 3)
            if configs[c][0] == vr.VR_MODE_ISO:
                r.synchronize()
                if kept is None:
                    kept = frame.clone()
                    hit_fraction[cam] = round(float((kept[..., :3] != bg).any(dim=-1).float().mean()), 4)
                same[f"{cam}/{c}"] = bool(torch.equal(frame, kept))
    samples = {case: [] for case in cases}
    for _ in range(a.rounds):
        for case in cases:
            samples[case].append(run(*case, a.frames))
    doc = {"source": "tools/iso_probe.py: HIP events around each march launch (vr_timing_read), ms per frame; "
                     "median and range over rounds, configurations alternating in one process",
           "device": torch.cuda.get_device_name(0), "volume": "MNI stand-in 182x218x182", "frame": [W, H, S],
           "iso_value": iso_value, "cal_max": cal, "rounds": a.rounds, "frames_per_round": a.frames,
           "iso_frames_equal": same, "surface_pixel_fraction": hit_fraction, "results": []}
    for (c, cam), v in samples.items():
        doc["results"].append({"config": c, "camera": cam, "ms_median": round(statistics.median(v), 4),
                               "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)})
    res = {(x["config"], x["camera"]): x for x in doc["results"]}
    doc["iso_ess_ert_over_mip_ess"] = {cam: round(res[("iso_ess_ert", cam)]["ms_median"] /
                                                  res[("mip_ess", cam)]["ms_median"], 3) for cam in cams}
    doc["iso_ess_ert_over_iso"] = {cam: round(res[("iso_ess_ert", cam)]["ms_median"] /
                                              res[("iso", cam)]["ms_median"], 3) for cam in cams}
    doc["mip_ess_spread_ms"] = {cam: round(res[("mip_ess", cam)]["ms_max"] - res[("mip_ess", cam)]["ms_min"], 4)
                                for cam in cams}
    doc["condition_iso_not_slower_than_mip_ess"] = {
        cam: bool(res[("iso_ess_ert", cam)]["ms_median"] <=
                  res[("mip_ess", cam)]["ms_median"] + doc["mip_ess_spread_ms"][cam]) for cam in cams}
    r.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
