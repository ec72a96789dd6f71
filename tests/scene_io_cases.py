"""One small saved scene in the three layouts eprecon_amd/scene_io.py reads, for the host and the GPU tests of the reader:
a 12 x 10 x 8 volume (unequal axes: a swapped axis shows) with 60 voxel rows, the corner cells (0,0,0) and (11,9,7) among
them, stored in a shuffled order; semantic is int64 in the dense and the legacy file and int32 in the sparse one."""
import os

import numpy as np

DIMS = (12, 10, 8)
N_ROWS = 60
ORIGIN = np.array([-1.0, 0.5, 0.25], np.float32)
VOXEL = 0.04


def rows():
    """-> (coords int32[60,3] shuffled, tsdf f32[60], semantic int64[60] in 1..19, instance int64[60])"""
    rng = np.random.default_rng(12)
    last = int(np.prod(DIMS)) - 1
    cells = np.concatenate([[0, last], 1 + rng.choice(last - 1, N_ROWS - 2, replace=False)])
    cells = cells[rng.permutation(N_ROWS)]
    coords = np.stack(np.unravel_index(cells, DIMS), 1).astype(np.int32)
    assert (np.diff(cells) < 0).any() and len(np.unique(cells)) == N_ROWS          # not in raster order, no twins
    tsdf = rng.uniform(-0.9, 0.9, N_ROWS).astype(np.float32)
    return coords, tsdf, rng.integers(1, 20, N_ROWS).astype(np.int64), rng.integers(0, 7, N_ROWS).astype(np.int64)


def volumes():
    """the dense truth: tsdf f32 (default 1), semantic, instance int32 (default 0)"""
    c, tsdf, sem, ins = rows()
    at = tuple(c.T.astype(np.int64))
    vols = np.ones(DIMS, np.float32), np.zeros(DIMS, np.int32), np.zeros(DIMS, np.int32)
    for vol, values in zip(vols, (tsdf, sem, ins)):
        vol[at] = values
    return vols


def write_layouts(root):
    """-> {"dense": path, "sparse": path, "legacy": path}"""
    os.makedirs(root, exist_ok=True)
    c, tsdf, sem, ins = rows()
    vt, vs, vi = volumes()
    paths = {k: os.path.join(str(root), k + ".npz") for k in ("dense", "sparse", "legacy")}
    np.savez_compressed(paths["dense"], origin=ORIGIN, voxel_size=VOXEL, tsdf=vt, semantic=vs.astype(np.int64), instance=vi)
    np.savez_compressed(paths["sparse"], origin=ORIGIN, voxel_size=VOXEL, dims=np.array(DIMS), sparse_coords=c, sparse_tsdf=tsdf,
                        sparse_semantic=sem.astype(np.int32), sparse_instance=ins.astype(np.int32))
    np.savez_compressed(paths["legacy"], origin=ORIGIN, voxel_size=VOXEL, dims=np.array(DIMS), coords=c, tsdf=tsdf, semantic=sem,
                        instance=ins)
    return paths
