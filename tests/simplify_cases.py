"""Meshes for the simplification tests, numpy only (tests/test_simplify_host.py, tests/test_simplify_gpu.py).  Every builder
returns (vertices float32[N,3], faces int32[M,3])."""
import numpy as np


def fan(triangles, collapse=False):
    """A fan of `triangles` triangles around a hub that is alone in its cell (cell size 1, origin 0).  The rim winds 0.9 of a
    turn at radius 2 with a wobble in z, so the hub's planes differ; collapse: the whole rim sits in the one cell (1, 0, 0)."""
    hub = np.array([0.5, 0.5, 0.5])
    t = 2.0 * np.pi * 0.9 * np.arange(triangles + 1) / max(triangles, 1)
    if collapse:
        rim = np.array([1.5, 0.5, 0.5]) + 0.3 * np.stack([0.2 * np.sin(2 * t), np.cos(t), np.sin(t)], 1)
    else:
        rim = hub + 2.0 * np.stack([np.cos(t), np.sin(t), 0.3 * np.sin(3 * t)], 1)
    verts = np.concatenate([hub[None], rim]).astype(np.float32)
    i = np.arange(triangles)
    return verts, np.stack([np.zeros_like(i), 1 + i, 2 + i], 1).astype(np.int32)


def grid(xs, ys, height):
    """the height field z = height(x, y) over the grid xs x ys, two triangles a quad"""
    x, y = np.meshgrid(np.asarray(xs, np.float64), np.asarray(ys, np.float64), indexing="ij")
    verts = np.stack([x, y, height(x, y)], -1).reshape(-1, 3).astype(np.float32)
    nx, ny = len(xs), len(ys)
    i, j = np.meshgrid(np.arange(nx - 1), np.arange(ny - 1), indexing="ij")
    a, b, c, d = (i * ny + j).ravel(), ((i + 1) * ny + j).ravel(), ((i + 1) * ny + j + 1).ravel(), (i * ny + j + 1).ravel()
    faces = np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)]).astype(np.int32)
    return verts, faces


def dyadic_lattice():
    """cell = 0.25: a height field on the multiples of 2^-4 in [-0.5, 0.5]^2, heights multiples of 2^-4 of both signs: every
    fifth row and column lies exactly on a cell face"""
    s = np.arange(-8, 9) / 16.0
    return grid(s, s, lambda x, y: (np.round(x * 16) * np.round(y * 16) % 5 - 2) / 16.0)


def dihedral():
    """two planes z = 0.3 -+ 0.5 x meeting in the ridge x = 0, z = 0.3; with cell 1 and origin (-0.5, -0.5, -0.5) the cell
    (0, 0, 0) holds nine vertices, three of them on the ridge"""
    s = -1.6 + 0.4 * np.arange(9)
    return grid(s, s, lambda x, y: 0.3 - 0.5 * np.abs(x))


def block_labels(vertices, seed, block=4.0):
    """seeded labels constant on blocks of `block` units: (semantic in [0, 5), instance in [0, 4)) int32[N] each"""
    rng = np.random.default_rng(seed)
    b = np.floor(np.asarray(vertices, np.float64) / block).astype(np.int64)
    b -= b.min(0)
    dims = b.max(0) + 1
    flat = (b[:, 0] * dims[1] + b[:, 1]) * dims[2] + b[:, 2]
    sem, ins = rng.integers(0, 5, int(np.prod(dims))), rng.integers(0, 4, int(np.prod(dims)))
    return sem[flat].astype(np.int32), ins[flat].astype(np.int32)


def seeded_colors(n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, 3)).astype(np.uint8)
