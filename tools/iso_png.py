"""The visual check of VR_MODE_ISO: avg152 at 300 x 300 x 300 through vr_render_png, default and reset
camera, an ISO frame (skin at --skin, a brighter surface at --inner) beside the VR_MODE_MIP frame of
the same view (needs a GPU).

    python tools/iso_png.py --out /tmp/iso_png
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
    ap.add_argument("--out", required=True, help="directory the six PNGs are written to")
    ap.add_argument("--skin", type=float, default=40.0, help="isovalue of the outer surface, voxel units")
    ap.add_argument("--inner", type=float, default=100.0, help="isovalue of the inner surface, voxel units")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    vol, hdr = volumes.avg152()
    W = H = S = 300
    E, T = vr.VR_FLAG_ESS, vr.VR_FLAG_ERT
    frames = (("iso_skin", vr.VR_MODE_ISO, a.skin, (0.95, 0.8, 0.7)),
              ("iso_inner", vr.VR_MODE_ISO, a.inner, (0.9, 0.9, 0.85)),
              ("mip", vr.VR_MODE_MIP, None, None))
    with vr.VolumeRenderer(vol, hdr["cal_max"], device=0) as r:
        for name, mode, iso, rgb in frames:
            if iso is not None:
                r.set_isosurface(iso, rgb)
            for cname, cam in (("default", vr.default_camera(W, H)), ("reset", vr.reset_camera())):
                p = vr.default_params(W, H, S, mode=mode, flags=E | T)
                p.shade_ambient, p.shade_diffuse, p.shade_specular, p.shade_shininess = 0.25, 0.7, 0.2, 24.0
                path = os.path.join(a.out, f"avg152_{name}_{cname}_300.png")
                rc = vr.lib().vr_render_png(r._ctx, C.byref(p), C.byref(cam), renderer.VR_ORIENT_TEST_DISPLAY,
                                            path.encode())
                if rc != 0:
                    raise SystemExit(f"vr_render_png failed with {rc} for {path}")
                print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
