"""The visual check of VR_MODE_MIP: avg152 at 300 x 300 x 300 through vr_render_png, default and reset
camera, a MIP frame beside the VR_MODE_DVR frame of the same view (needs a GPU).

    python tools/mip_png.py --out /tmp/mip_png
"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import volumerenderingproject_amd as vr  # noqa: E402
from volumerenderingproject_amd import renderer, volumes  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True, help="directory the four PNGs are written to")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    vol, hdr = volumes.avg152()
    W = H = S = 300
    with vr.VolumeRenderer(vol, hdr["cal_max"], device=0) as r:
        for name, mode in (("mip", vr.VR_MODE_MIP), ("dvr", vr.VR_MODE_DVR)):
            for cname, cam in (("default", vr.default_camera(W, H)), ("reset", vr.reset_camera())):
                p = vr.default_params(W, H, S, mode=mode)
                path = os.path.join(a.out, f"avg152_{name}_{cname}_300.png")
                rc = vr.lib().vr_render_png(r._ctx, C.byref(p), C.byref(cam), renderer.VR_ORIENT_TEST_DISPLAY,
                                            path.encode())
                if rc != 0:
                    raise SystemExit(f"vr_render_png failed with {rc} for {path}")
                print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
