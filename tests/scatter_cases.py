"""Small designed groups for the scatter's phase 2 (tests/test_gpu_scatter_mfma.py and its child tests/run_scatter_cases.py).

The frame is lattice_design's: every image begins with the unlinked points (0,0,0) and (64,64,64), every other point lies in
[0,64]^3, and with lattice_design.OPTIONS level 0 has spacing 8 and origin -24: a coordinate x lies in the 0-based cell
floor(x / 8) + 2 of 12 per axis.  With bricks of 4^3 cells an axis splits into [0,16), [16,48) and [48,64]; with bricks of 8^3
(the 11^3 tile) into [0,48) and [48,64].  Images 1 and 2 are copies of image 0 moved by less than 0.02 per axis and point k is
linked to point k in the blocks (0,1), (0,2), (1,2): every link is shorter than 0.1, so its weight is exactly 1 and a linked
point has sWeight 2.  Points stay 0.05 away from the faces of their cell, so the copies lie in the same cells.

A scatter block is a run of at most 384 points of one (image, brick), unlinked points included, in cell order; phase 2 takes
its live points (sWeight != 0) 64 to a batch and four to a group.
"""
import numpy as np

import lattice_design as ld

OPTIONS = ld.OPTIONS
ALPHA = 1.0
STEPS = 3
# bricks of 4^3 cells, (bx, by, bz) -> points of image 0 in it: the group-of-four remainders, the batch edge, the chunk edge
SIZES = {(1, 0, 0): 1, (0, 1, 0): 3, (0, 0, 1): 4, (1, 1, 0): 5, (1, 0, 1): 63, (0, 1, 1): 64, (1, 1, 1): 65, (2, 1, 1): 384,
         (1, 2, 1): 385}
ONE_CELL = ((3, 0, 0), 150)              # cell (x / 8 per axis) and points: one chain over three batches
TWO_CELLS = (((0, 3, 0), 70), ((0, 4, 0), 30))      # the second batch begins inside the first cell's run, then changes once
SPARSE_BRICK = ((0, 0, 1), 90)           # every third point of this brick has no link: holes in the middle of the batches
STRAY_BOX = ([16.0] * 3, [48.0] * 3)     # lattice over [16,48]^3: spacing 8, origin 0; a linked point at x < 8 is a stray
STRAY_POINT = (4.0, 30.0, 30.0)
# case: (group, brick edge, box of the lattice or None for the group's own)
CASES = {"sizes_brick4": ("sizes", 4, None), "sizes_brick8": ("sizes", 8, None), "cells_brick4": ("cells", 4, None),
         "cells_brick8": ("cells", 8, None), "stray": ("stray", 4, STRAY_BOX)}

_EDGES4 = ((0.0, 16.0), (16.0, 48.0), (48.0, 64.0))


def _in_brick(rng, brick, n):
    """n points in cells of the brick, 0.05 from every cell face."""
    lo = np.array([_EDGES4[b][0] for b in brick]); hi = np.array([_EDGES4[b][1] for b in brick])
    cell = rng.integers((lo / 8).astype(int), (hi / 8).astype(int), (n, 3))
    return 8.0 * cell + rng.uniform(0.05, 7.95, (n, 3))


def _in_cell(rng, cell, n):
    return 8.0 * np.array(cell, np.float64) + rng.uniform(0.05, 7.95, (n, 3))


def image0(group, rng):
    """(points of image 0 behind the frame [n, 3] f64, linked [n] bool)."""
    if group == "sizes":
        pts = np.concatenate([_in_brick(rng, b, n) for b, n in SIZES.items()])
        return pts, np.ones(len(pts), bool)
    if group == "cells":
        own = np.stack(np.meshgrid(np.arange(2, 6), np.arange(2, 6), np.arange(2, 6), indexing="ij"), axis=-1).reshape(-1, 3)
        parts = [8.0 * own + rng.uniform(0.05, 7.95, (64, 3)),                # brick (1,1,1): every point in a cell of its own
                 _in_cell(rng, *ONE_CELL)]
        parts += [_in_cell(rng, c, n) for c, n in TWO_CELLS]
        parts.append(_in_brick(rng, *SPARSE_BRICK))
        pts = np.concatenate(parts)
        linked = np.ones(len(pts), bool)
        linked[len(pts) - SPARSE_BRICK[1] + 1::3] = False
        return pts, linked
    if group == "stray":
        pts = np.concatenate([rng.uniform(17.0, 47.0, (200, 3)), np.array([STRAY_POINT])])
        return pts, np.ones(len(pts), bool)
    raise KeyError(group)


def build(group, seed=31):
    """(point_offset, xyz f32 [P, 3], blocks, linked [points of an image] bool) of a group of three images."""
    rng = np.random.default_rng(seed)
    f32 = np.float32
    frame = np.array([[0, 0, 0], [64, 64, 64]], f32)
    pts, linked = image0(group, rng)
    img0 = np.concatenate([frame, pts.astype(f32)])
    linked = np.concatenate([[False, False], linked])
    n = len(img0)
    images = [img0]
    for sign in (1.0, -1.0):
        shift = sign * 0.0115 * np.array([1.0, -1.0, 1.0]) + rng.uniform(-0.008, 0.008, (n, 3))
        moved = (img0.astype(np.float64) + shift).astype(f32)
        moved[:2] = frame
        images.append(moved)
    po = np.concatenate([[0], np.cumsum([len(a) for a in images])])
    k = np.nonzero(linked)[0].astype(np.uint32)
    return po, np.concatenate(images), [(0, 1, k, k), (0, 2, k, k), (1, 2, k, k)], linked


_pairs = {}


def pairs(group):
    from frog_amd.pairs import Pairs
    if group not in _pairs:
        po, xyz, blocks, _ = build(group)
        _pairs[group] = Pairs.from_arrays(po, xyz, blocks)
    return _pairs[group]
