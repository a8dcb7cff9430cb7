"""The visual check of VR_MODE_SDVR: the MNI stand-in at 400 x 400 x 400 through vr_render_png, default and
reset camera, the shaded frame beside the flat VR_MODE_DVR frame of the same view (needs a GPU).

    python tools/sdvr_png.py --out /tmp/sdvr_png
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
    ap.add_argument("--size", type=int, default=400, help="width = height = samples per ray")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    vol, cal = volumes.mni152_standin()
    W = H = S = a.size
    E, T = vr.VR_FLAG_ESS, vr.VR_FLAG_ERT
    with vr.VolumeRenderer(vol, cal, device=0) as r:
        for name, mode in (("sdvr", vr.VR_MODE_SDVR), ("dvr", vr.VR_MODE_DVR)):
            for cname, cam in (("default", vr.default_camera(W, H)), ("reset", vr.reset_camera())):
                p = vr.default_params(W, H, S, mode=mode, flags=E | T)
                p.shade_ambient, p.shade_diffuse, p.shade_specular, p.shade_shininess = 0.25, 0.7, 0.2, 24.0
                path = os.path.join(a.out, f"mni_{name}_{cname}_{a.size}.png")
                rc = vr.lib().vr_render_png(r._ctx, C.byref(p), C.byref(cam), renderer.VR_ORIENT_TEST_DISPLAY,
                                            path.encode())
                if rc != 0:
                    raise SystemExit(f"vr_render_png failed with {rc} for {path}")
                print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
