"""The visual check of VR_MODE_CDVR: avg152 at 300 x 300 x 300 through vr_render_png, default and reset
camera, under a skin-to-bone ramp (opacity rising through soft tissue, colour blending from skin tones to
bone white) beside the VR_MODE_DVR frame of the same view under the default interval TF (needs a GPU).

    python tools/cmap_png.py --out /tmp/cmap_png
"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import volumerenderingproject_amd as vr  # noqa: E402
from volumerenderingproject_amd import renderer, volumes  # noqa: E402

SKIN_BONE = [(0.0, (0.0, 0.0, 0.0, 0.0)), (40.0, (0.0, 0.0, 0.0, 0.0)), (90.0, (0.85, 0.55, 0.45, 0.03)),
             (150.0, (0.9, 0.7, 0.6, 0.08)), (200.0, (1.0, 0.95, 0.85, 0.5)), (255.0, (1.0, 1.0, 1.0, 0.9))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True, help="directory the four PNGs are written to")
    ap.add_argument("--size", type=int, default=300, help="width = height = samples per ray")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    vol, hdr = volumes.avg152()
    W = H = S = a.size
    E, T = vr.VR_FLAG_ESS, vr.VR_FLAG_ERT
    with vr.VolumeRenderer(vol, hdr["cal_max"], device=0) as r:
        r.set_colormap(SKIN_BONE)
        for name, mode in (("cdvr", vr.VR_MODE_CDVR), ("dvr", vr.VR_MODE_DVR)):
            for cname, cam in (("default", vr.default_camera(W, H)), ("reset", vr.reset_camera())):
                p = vr.default_params(W, H, S, mode=mode, flags=E | T)
                path = os.path.join(a.out, f"avg152_{name}_{cname}_{a.size}.png")
                rc = vr.lib().vr_render_png(r._ctx, C.byref(p), C.byref(cam), renderer.VR_ORIENT_TEST_DISPLAY,
                                            path.encode())
                if rc != 0:
                    raise SystemExit(f"vr_render_png failed with {rc} for {path}")
                print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
