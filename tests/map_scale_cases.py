"""Map-scale scenes of tests/test_map_scale_gpu.py, built deterministically from fixed seeds; tests/test_map_scale_cases.py holds the properties
that make them meaningful on the CPU.  No test lives here.

The sizes are the smallest that cross the branches small scenes never take: scan.hpp scans its tile sums (a tile is 4096 entries) in chunks
of 1024 tiles with a serial carry, so only an array of more than 1024 x 4096 = 4 194 304 entries uses the carry; find_sub searches the
sub-map offsets, where empty sub-maps share an offset; edit_seed_final_kernel strides over the partial minima only beyond 256 blocks of 256
candidates.

Scene A  "many sub-maps, just past one scan chunk": 71 sub-maps of 0, 1, 32 x 65 536, 0, 0, 255, 32 x 65 536, 4097 and 0 points, 4 198 657 in
         all; the flag array has one entry more, 1026 tiles.  FP32 clouds, except the 255- and the 4097-point ones, which keep FP64 points.
         Every sub-map has a rigid pose of its own (rotations of order 0.5 rad, translations of order 20 m); the points are uniform in a cube
         of edge 5.6 m around CENTER in the world frame, of which the selection volumes of PREDICATES_A and the ball hold 1 - 10 %, and are
         then mapped into their sub-map's frame.  Points strictly inside every selection volume sit at the concatenated indices FORCED.
Scene B  "one large cloud": 4 198 657 FP32 points with normals and covariances; component 0 of every array is the point's index, the rest is
         random, so that a misplaced row shows in every array.
Scene C  "more than 256 seed blocks": a jittered planar lattice of 260 x 260 points, spacing 0.05 m, through CENTER (sub-map 0) and a second
         patch of 10 x 260 behind a gap of 0.5 m (sub-map 1), both under the identity and all inside the window: 70 200 candidates in 275
         blocks.  Candidates 7 and 65 600 -- blocks 0 and 256, which the same thread of the final kernel folds -- are CENTER + (2^-6, 0, 0) and
         CENTER + (0, 2^-6, 0): the same squared distance 2^-12, exactly, and smaller than every other point's.
"""
import numpy as np

import map_edit_restatement as R
from glim_amd.se3 import se3_exp

CENTER = R.CENTER
TILE, CHUNK_TILES = 4096, 1024
CHUNK = TILE * CHUNK_TILES  # 4 194 304: the entries one chunk of the tile-sum scan covers

# ---- scene A -------------------------------------------------------------------------------------------------------------------------------
SIZES_A = [0, 1] + [65536] * 32 + [0, 0, 255] + [65536] * 32 + [4097, 0]
TOTAL_A = 4198657
EXACT_A = (36, 69)  # the FP64 clouds: the 255- and the 4097-point one
FORCED = (0, 4095, 4096, CHUNK - 1, CHUNK, TOTAL_A - 1)
HALF_EDGE = 2.8
BALL_RADIUS = 1.0  # of the bundle-adjustment ball selection

# name -> (mode, keyword arguments of the device call, arguments of map_edit_restatement.select behind the matrices)
PREDICATES_A = {
    "box": (R.BOX, dict(model_matrix=R.MODEL), (R.BOX,)),
    "sphere": (R.SPHERE, dict(model_matrix=R.MODEL), (R.SPHERE,)),
    "window": (R.WINDOW, dict(center=CENTER, resolution=0.5, window=1), (R.WINDOW, CENTER, 0.0, 0.5, 1)),
    "window_ball": (R.WINDOW_BALL, dict(center=CENTER, radius=0.8), (R.WINDOW_BALL, CENTER, 0.8)),
}
EVERYTHING = (R.WINDOW, dict(center=CENTER), (R.WINDOW, CENTER))  # cells of 2 m, 5 to either side: the cube lies inside
NOTHING = (R.WINDOW_BALL, dict(center=[1000.0, 1000.0, 1000.0], radius=0.8), (R.WINDOW_BALL, np.array([1000.0, 1000.0, 1000.0]), 0.8))


def local_matrices(model_matrix, poses):
    """api.edit_local_matrices, restated: inv(model matrix) T_world_submap, 3 x 4"""
    inv = np.linalg.inv(np.asarray(model_matrix, dtype=np.float64).reshape(4, 4))
    return [(inv @ T)[:3, :4].copy() for T in poses]


def matrices_a(mode, poses):
    return local_matrices(R.MODEL, poses) if mode in (R.BOX, R.SPHERE) else poses


def owner(sizes, index):
    """(sub-map, point) of a concatenated index: the LAST sub-map whose offset is <= index"""
    off = np.concatenate([[0], np.cumsum(sizes)])
    s = int(np.searchsorted(off[:-1], index, side="right")) - 1
    return s, int(index - off[s])


def scene_a(seed=2024):
    """-> {clouds, poses, exact, sizes, total, forced}: clouds are FP64 arrays holding what the device holds (the FP32 clouds' points are
    rounded here, as clone() rounds them); exact[s]: sub-map s is an FP64 cloud; forced: the (sub-map, point) pairs of FORCED."""
    rng = np.random.default_rng(seed)
    S = len(SIZES_A)
    poses = [se3_exp(np.concatenate([rng.normal(size=3) * 0.5, rng.normal(size=3) * 20.0])) for _ in range(S)]
    forced = [owner(SIZES_A, i) for i in FORCED]
    clouds = []
    for s, (n, T) in enumerate(zip(SIZES_A, poses)):
        w = CENTER + rng.uniform(-HALF_EDGE, HALF_EDGE, size=(n, 3))
        for k, (fs, fj) in enumerate(forced):
            if fs == s:
                w[fj] = CENTER + 0.01 * (k + 1) * np.array([1.0, -1.0, 1.0])
        p = (w - T[:3, 3]) @ T[:3, :3]
        if s not in EXACT_A:
            p = p.astype(np.float32).astype(np.float64)
        clouds.append(p.reshape(-1, 3))
    return {"clouds": clouds, "poses": poses, "exact": [s in EXACT_A for s in range(S)], "sizes": list(SIZES_A), "total": int(sum(SIZES_A)),
            "forced": np.array(forced, dtype=np.int32)}


def all_pairs(sizes):
    """every (sub-map, point) in order: what a predicate that selects everything returns (the empty sub-maps do not appear)"""
    return np.concatenate([np.stack([np.full(n, s), np.arange(n)], axis=1) for s, n in enumerate(sizes)]).astype(np.int32)


# ---- scene B -------------------------------------------------------------------------------------------------------------------------------
N_B = TOTAL_A


def scene_b(seed=2025):
    """-> {points n x 3, normals n x 3, covs n x 3 x 3 (symmetric)}, FP32"""
    rng = np.random.default_rng(seed)
    idx = np.arange(N_B, dtype=np.float32)  # exact: N_B < 2^24
    points = rng.random((N_B, 3), dtype=np.float32)
    normals = rng.random((N_B, 3), dtype=np.float32)
    six = rng.random((N_B, 6), dtype=np.float32)
    points[:, 0] = normals[:, 0] = six[:, 0] = idx
    covs = six[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(N_B, 3, 3)
    return {"points": points, "normals": normals, "covs": np.ascontiguousarray(covs)}


def removal_indices_b(n=N_B):
    """every third index, the tile and chunk boundaries, a run of 5000 across the chunk boundary, duplicates; unsorted"""
    idx = np.concatenate([np.arange(0, n, 3), [0, 4095, 4096, CHUNK - 1, CHUNK, n - 1], np.arange(CHUNK - 2500, CHUNK + 2500), np.arange(0, n, 3)[:1000],
                          [CHUNK, CHUNK, n - 1]])
    return idx[::-1].astype(np.int32)


def second_removal_indices_b(n):
    """for the result of the first removal (below one chunk): every fifth index, both ends, tile boundaries, duplicates"""
    return np.concatenate([np.arange(0, n, 5), [0, 4095, 4096, 8191, 8192, n - 1, n - 1]]).astype(np.int32)


# ---- scene C -------------------------------------------------------------------------------------------------------------------------------
SPACING_C, THRESHOLD_C, DILATION_C, GAP_C = 0.05, 0.15, 0.25, 0.5
SIDE_C, PATCH_ROWS_C = 260, 10
TIE_C = (7, 65600)  # candidate indices: blocks 0 and 256 of 256 candidates
TIE_QQ = 2.0 ** -12


def scene_c(seed=2026):
    """-> {clouds (2, FP64), poses (identities), tie}"""
    rng = np.random.default_rng(seed)
    g = (np.arange(SIDE_C) - SIDE_C / 2 + 0.5) * SPACING_C  # CENTER sits in the middle of a lattice cell
    main = np.stack(np.meshgrid(g, g, [0.0], indexing="ij"), axis=-1).reshape(-1, 3)
    gx = g[-1] + GAP_C + np.arange(PATCH_ROWS_C) * SPACING_C
    patch = np.stack(np.meshgrid(gx, g, [0.0], indexing="ij"), axis=-1).reshape(-1, 3)
    clouds = []
    for lattice in (main, patch):
        jitter = np.concatenate([rng.uniform(-0.01, 0.01, size=(len(lattice), 2)), rng.uniform(-0.005, 0.005, size=(len(lattice), 1))], axis=1)
        clouds.append(CENTER + lattice + jitter)
    clouds[0][TIE_C[0]] = CENTER + np.array([2.0 ** -6, 0.0, 0.0])
    clouds[0][TIE_C[1]] = CENTER + np.array([0.0, 2.0 ** -6, 0.0])
    return {"clouds": clouds, "poses": [np.eye(4), np.eye(4)], "tie": TIE_C}
