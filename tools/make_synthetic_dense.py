#!/usr/bin/env python3
"""Writes a synthetic dense folder in the reference's layout (pair.txt, cams/%08d_cam.txt, images/%08d.pgm|jpg) from the
analytic scene generator: `num_views` cameras on a ring looking at slanted, textured planes.

  python tools/make_synthetic_dense.py <folder> --width 1920 --height 1080 --views 16 --src 10 [--textureless 0.2] [--jpeg] [--hard] [--gt] [--masks 0.3]

--hard: the synth.HARD scene (slabs in front of the planes, per-view gain / offset, sources aiming off the target).
--masks FRACTION: also writes masks/%08d.pgm|jpg (0 = masked out, 255 = process), seeded: a band of "sky" along the top plus a few blobs, about FRACTION of every frame.
--gt:   also writes gt/%08d.npy (+ _normal.npy, _textured.npy), the analytic z-depth, world-frame normal and has-texture mask of every view (tools/jacobi_vs_gs.py compares both orders of views against it).
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synthetic_mask(width, height, fraction, seed, view):
    """uint8 [height, width], 0 = masked out, 255 = process: a band of "sky" along the top with a wavy lower edge (two thirds of
    `fraction`) plus a few elliptic blobs (the rest, less what overlaps); a function of the arguments alone."""
    rng = np.random.RandomState((int(seed) * 1000003 + int(view) * 7919 + 17) % (2 ** 31 - 1))
    ys, xs = np.mgrid[0:height, 0:width]
    band = (2.0 / 3.0) * fraction * height
    edge = band * (1.0 + 0.25 * np.sin(2.0 * np.pi * (xs / float(width) * rng.uniform(1.0, 3.0) + rng.uniform())))
    out = ys < edge
    blobs = 3
    area = (fraction / 3.0) * width * height / blobs
    for _ in range(blobs):
        cx, cy = rng.uniform(0.1, 0.9) * width, rng.uniform(0.4, 0.9) * height
        aspect = rng.uniform(0.6, 1.6)
        rx, ry = np.sqrt(area / np.pi * aspect), np.sqrt(area / np.pi / aspect)
        out |= ((xs - cx) / rx) ** 2 + ((ys - cy) / ry) ** 2 < 1.0
    return np.where(out, 0, 255).astype(np.uint8)


def write_masks(folder, width, height, num_views, fraction, seed=0, jpeg=False):
    os.makedirs(os.path.join(folder, "masks"), exist_ok=True)
    for i in range(num_views):
        m = synthetic_mask(width, height, fraction, seed, i)
        if jpeg:
            from PIL import Image
            Image.fromarray(m, "L").save(os.path.join(folder, "masks", "%08d.jpg" % i), quality=95)
        else:
            with open(os.path.join(folder, "masks", "%08d.pgm" % i), "wb") as f:
                f.write(b"P5\n%d %d\n255\n" % (width, height) + m.tobytes())


def write_dense_folder(folder, synth, width, height, num_views, num_src, seed=0, textureless=0.0, jpeg=False, device="cpu", hard=False, gt=False):
    os.makedirs(os.path.join(folder, "images"), exist_ok=True)
    os.makedirs(os.path.join(folder, "cams"), exist_ok=True)
    sc = synth.make_scene(width, height, num_views - 1, seed=seed, textureless=textureless, device=device, keep_view_depths=gt,
                          **(synth.HARD if hard else {}))
    imgs = sc.images_numpy()
    if gt:
        os.makedirs(os.path.join(folder, "gt"), exist_ok=True)
        for i in range(num_views):
            np.save(os.path.join(folder, "gt", "%08d.npy" % i), sc.view_depths[i].detach().cpu().numpy())
            np.save(os.path.join(folder, "gt", "%08d_normal.npy" % i), sc.view_normals[i].detach().cpu().numpy())
            np.save(os.path.join(folder, "gt", "%08d_textured.npy" % i), sc.view_textured[i].detach().cpu().numpy())
    for i in range(num_views):
        a = imgs[i].astype(np.uint8)
        if jpeg:
            from PIL import Image
            Image.fromarray(a, "L").save(os.path.join(folder, "images", "%08d.jpg" % i), quality=95)
        else:
            with open(os.path.join(folder, "images", "%08d.pgm" % i), "wb") as f:
                f.write(b"P5\n%d %d\n255\n" % (width, height) + a.tobytes())
        R, t, K = sc.R[i].reshape(3, 3), sc.t[i], sc.K[i].reshape(3, 3)
        txt = "extrinsic\n"
        for r in range(3):
            txt += "%.9g %.9g %.9g %.9g\n" % (R[r, 0], R[r, 1], R[r, 2], t[r])
        txt += "0 0 0 1\n\nintrinsic\n"
        for r in range(3):
            txt += "%.9g %.9g %.9g\n" % (K[r, 0], K[r, 1], K[r, 2])
        txt += "\n%.9g 0.01 192 %.9g\n" % (sc.depth_min, sc.depth_max)
        with open(os.path.join(folder, "cams", "%08d_cam.txt" % i), "w") as f:
            f.write(txt)
    pair = "%d\n" % num_views
    for i in range(num_views):
        srcs = sorted((j for j in range(num_views) if j != i), key=lambda j: (abs(j - i), j))[:num_src]
        pair += "%d\n%d %s\n" % (i, len(srcs), " ".join("%d %.1f" % (j, 100.0 - k) for k, j in enumerate(srcs)))
    with open(os.path.join(folder, "pair.txt"), "w") as f:
        f.write(pair)
    return sc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("folder")
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--views", type=int, default=5)
    ap.add_argument("--src", type=int, default=4)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--textureless", type=float, default=0.0)
    ap.add_argument("--jpeg", action="store_true")
    ap.add_argument("--hard", action="store_true")
    ap.add_argument("--gt", action="store_true")
    ap.add_argument("--masks", type=float, default=0.0, metavar="FRACTION", help="also write masks/ with about this share of every frame masked out")
    args = ap.parse_args()
    import __graft_entry__ as ge
    ge.load_package()
    from apd_mvs_amd import synth
    import torch
    dev = "cuda" if torch.cuda.is_available() else "cpu"
    write_dense_folder(args.folder, synth, args.width, args.height, args.views, args.src, args.seed, args.textureless, args.jpeg, dev, hard=args.hard, gt=args.gt)
    if args.masks > 0:
        write_masks(args.folder, args.width, args.height, args.views, args.masks, args.seed, args.jpeg)
    print("wrote", args.folder)


if __name__ == "__main__":
    main()
