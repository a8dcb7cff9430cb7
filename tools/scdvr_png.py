"""The visual check of VR_MODE_SCDVR: avg152 at 300 x 300 x 300 through vr_render_png, default and reset
camera, under the skin-to-bone ramp of tools/cmap_png.py with G = edges (flat tissue transparent, full
weight at strong boundaries) and with G = unit, beside the VR_MODE_CDVR frame of the same view (needs a GPU).

    python tools/scdvr_png.py --out /tmp/scdvr_png
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
EDGES = [(1.5, 0.0), (8.0, 0.25), (80.0, 1.0)]
UNIT = [(0.0, 1.0)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True, help="directory the six PNGs are written to")
    ap.add_argument("--size", type=int, default=300, help="width = height = samples per ray")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    vol, hdr = volumes.avg152()
    W = H = S = a.size
    E, T = vr.VR_FLAG_ESS, vr.VR_FLAG_ERT
    with vr.VolumeRenderer(vol, hdr["cal_max"], device=0) as r:
        r.set_colormap(SKIN_BONE)
        for name, mode, g in (("scdvr_edges", vr.VR_MODE_SCDVR, EDGES), ("scdvr_unit", vr.VR_MODE_SCDVR, UNIT),
                              ("cdvr", vr.VR_MODE_CDVR, UNIT)):
            r.set_gradient_opacity(g)
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
