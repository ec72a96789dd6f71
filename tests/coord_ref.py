"""Dictionary model of the coordinate kernels (hash grid, unique numbering and its hierarchy, kernel maps, transposed map, rank
volume) and the fixture sets the limit tests run on.

The model works on tuples of Python ints and never packs a key: a voxel is the tuple (b, x, y, z) itself and a table is a dict.
oracle/sparse.py packs keys with the kernels' own shifts and has no range rule, so past the limit it aliases exactly as a wrong
kernel would; this model cannot.  The range rule is the documented one (csrc/hashgrid.hpp, sparse.check_hash_status): batch
0 .. 14 and |coordinate| <= 2^19 - 2 after quantising; anything else is refused (status bit 0) and the row drops out.

test_coord_ref.py (host) pins the model to oracle/sparse.py on ordinary inputs and checks that the fixture sets below hold every
event they are built for; test_coord_limits_gpu.py runs the kernels on the same sets.
"""
import numpy as np

LIMIT = 2 ** 19 - 2       # the largest |coordinate| a key holds
MAX_BATCH = 14
STATUS_RANGE = 1          # status bit 0: a key out of range


def rows_of(a):
    """int rows of an array (or any nested sequence) as a list of tuples of Python ints"""
    return [tuple(int(v) for v in r) for r in (a.tolist() if hasattr(a, "tolist") else a)]


def in_range(b, x, y, z):
    return 0 <= b <= MAX_BATCH and abs(x) <= LIMIT and abs(y) <= LIMIT and abs(z) <= LIMIT


def quantise(row, q):
    b, x, y, z = row
    return (b, (x // q) * q, (y // q) * q, (z // q) * q)


def unique_first(rows, q=1):
    """-> (unique rows in first-occurrence order, inverse (-1: refused), dict key -> id, status).  Quantise, then test the range."""
    uniq, inverse, ids, status = [], [], {}, 0
    for row in rows:
        key = quantise(row, q)
        if not in_range(*key):
            status |= STATUS_RANGE
            inverse.append(-1)
            continue
        if key not in ids:
            ids[key] = len(uniq)
            uniq.append(key)
        inverse.append(ids[key])
    return uniq, inverse, ids, status


def lookup(ids, rows, q=1):
    """id of every (quantised) row, -1 when absent or refused; a query never touches a status"""
    out = []
    for row in rows:
        key = quantise(row, q)
        out.append(ids.get(key, -1) if in_range(*key) else -1)
    return out


def offsets(ksize):
    if ksize == 3:      # x fastest
        return [(k % 3 - 1, (k // 3) % 3 - 1, k // 9 - 1) for k in range(27)]
    if ksize == 2:      # z fastest
        return [((k >> 2) & 1, (k >> 1) & 1, k & 1) for k in range(8)]
    raise ValueError(ksize)


def kernel_map(ids, rows, ksize, stride):
    """nbr[k][i] = id of rows[i] + offset_k * stride in `ids`, -1 when absent or out of range"""
    out = []
    for dx, dy, dz in offsets(ksize):
        line = []
        for b, x, y, z in rows:
            key = (b, x + dx * stride, y + dy * stride, z + dz * stride)
            line.append(ids.get(key, -1) if in_range(*key) else -1)
        out.append(line)
    return out


def transpose_map(rows, parent, fine_stride):
    """up[k][i] = parent[i] when fine row i is child k = 4 bx + 2 by + bz of its parent, else -1"""
    s = fine_stride
    up = [[-1] * len(rows) for _ in range(8)]
    for i, (_, x, y, z) in enumerate(rows):
        bx, by, bz = ((c - (c // (2 * s)) * (2 * s)) // s for c in (x, y, z))
        up[4 * bx + 2 * by + bz][i] = parent[i]
    return up


def on_grid(row, stride, dims):
    return all(c >= 0 and c % stride == 0 and c // stride < d for c, d in zip(row[1:], dims))


def grid_rank(rows, stride, dims):
    """-> (volume as a flat list over (x, y, z) cells with z fastest: the row on the cell or -1, number of rows off the grid).
    Two rows on one cell have no defined winner: the model refuses such a list."""
    gx, gy, gz = dims
    vol, off = [-1] * (gx * gy * gz), 0
    for i, row in enumerate(rows):
        if not on_grid(row, stride, dims):
            off += 1
            continue
        cell = ((row[1] // stride) * gy + row[2] // stride) * gz + row[3] // stride
        if vol[cell] != -1:
            raise ValueError(f"rows {vol[cell]} and {i} share a cell")
        vol[cell] = i
    return vol, off


def hierarchy(rows, levels):
    """level l numbers the unique rows of level l - 1 (level 0: `rows`) at quantum 2^l -> [(unique, inverse, ids, status)]"""
    out, src = [], rows
    for l in range(levels):
        out.append(unique_first(src, 1 << l))
        src = out[-1][0]
    return out


def first_rows(rows, q=1):
    """what a hash build answers: for every row the first row with the same (quantised) key, -1 for a refused row"""
    first, out = {}, []
    for i, row in enumerate(rows):
        key = quantise(row, q)
        out.append(first.setdefault(key, i) if in_range(*key) else -1)
    return out


# ---- fixture sets ----------------------------------------------------------------------------------------------------------
# Builders are deterministic; they return int32 arrays of (b, x, y, z) rows.

def ordinary_rows(n, extent, batch, seed, stride=1):
    """n distinct rows in [-extent, extent)^3 x [0, batch), multiples of `stride`, shuffled"""
    rng = np.random.default_rng(seed)
    c = rng.integers(-extent, extent, size=(n * 3, 3)) * stride
    b = rng.integers(0, batch, size=(n * 3, 1))
    rows = np.unique(np.concatenate([b, c], 1), axis=0)
    rng.shuffle(rows)
    assert len(rows) >= n
    return rows[:n].astype(np.int32)


def with_duplicates(rows, share, seed):
    """`rows` plus share * len(rows) repeats of rows drawn from it, shuffled"""
    rng = np.random.default_rng(seed)
    out = np.concatenate([rows, rows[rng.integers(0, len(rows), int(share * len(rows)))]])
    rng.shuffle(out)
    return out


def limit_rows():
    """the rows at the packing limit, without the ordinary ones (test_coord_ref.test_limit_set_holds_every_event lists the events)"""
    rows = []
    for axis in range(3):
        for sign in (1, -1):
            for mag in (LIMIT, LIMIT + 1):             # +-(2^19 - 2) accepted, +-(2^19 - 1) refused
                c = [3, -5, 7]
                c[axis] = sign * mag
                rows.append((axis % 2, *c))
    rows += [(14, 1, -3, 2), (15, 1, -3, 2)]             # the last batch a key holds, and the reserved one
    rows += [(0, 2, -9, 4), (1, 2, -9, 4)]               # one place in two batches
    rows += [(0, -7, -3, -1), (2, -1, -1, -1)]           # negative odd
    # a block in the corner (+LIMIT, +LIMIT, -LIMIT): neighbours on the inside, none on the outside
    rows += [(1, LIMIT - i, LIMIT - j, -LIMIT + k) for i in range(5) for j in range(3) for k in range(3)]
    return rows


def limit_set():
    """a few hundred rows: limit_rows mixed into ordinary ones, duplicated and shuffled.  Refused rows at q = 1, 2 and 4."""
    rows = np.concatenate([np.array(limit_rows(), np.int32), ordinary_rows(180, 6, 3, seed=101)])
    return with_duplicates(rows, 0.5, seed=102)


def clean_set():
    """the same mixture with every row inside the limit at q = 1, 2 and 4: status 0"""
    corner = [(1, LIMIT - 2 - i, LIMIT - 2 - j, -LIMIT + 2 + k) for i in range(5) for j in range(3) for k in range(3)]
    rows = np.concatenate([np.array(corner + [(14, 1, -3, 2), (0, -7, -3, -1)], np.int32), ordinary_rows(180, 6, 3, seed=103)])
    return with_duplicates(rows, 0.5, seed=104)


def accepted_set(q):
    """the unique accepted rows of limit_set at quantum q (multiples of q): what the map kernels run on at stride q"""
    return np.array(unique_first(rows_of(limit_set()), q)[0], np.int32)


def map_rows(n, stride):
    """exactly n distinct accepted rows at `stride` for the map kernels' block edge: rows at the limit first, ordinary ones behind"""
    pool = rows_of(np.concatenate([np.array(limit_rows(), np.int32), ordinary_rows(1500, 8, 3, seed=105 + stride, stride=stride)]))
    uniq = unique_first(pool, stride)[0]
    corner = [r for r in uniq if max(abs(c) for c in r[1:]) > LIMIT - 8]
    rest = [r for r in uniq if max(abs(c) for c in r[1:]) <= LIMIT - 8]
    rows = (corner[:8] + rest)[:n] if n > 1 else corner[:1]
    assert len(rows) == n
    return np.array(rows, np.int32)


ALIAS_STRIDE = 4


def alias_rows():
    """-> (rows, [(i, k, j)]): row i sits at +LIMIT on one axis, and its neighbour at offset k of the 3x3x3 map at ALIAS_STRIDE
    is out of range but packs — bias added, fields shifted, no range test — to the key of row j of the same set"""
    rows = [(0, LIMIT, 5, -7), (1, -LIMIT, 5, -7),        # +x: the carry runs into the batch field
            (2, 4, LIMIT, -7), (2, 5, -LIMIT, -7),        # +y: into x (the fields are OR-ed: the bit it lands on must be clear)
            (3, 5, -8, LIMIT), (3, 5, -7, -LIMIT),        # +z: into y
            (0, 1, 5, -7), (2, 4, LIMIT - 4, -7)]         # and two ordinary neighbours
    return np.array(rows, np.int32), [(0, 14, 1), (2, 16, 3), (4, 22, 5)]


def query_set():
    """queries against limit_set's table: its own rows, rows at and past the limit that are not in it, ordinary absent rows"""
    extra = [(0, LIMIT, LIMIT, LIMIT), (0, LIMIT + 1, 0, 0), (0, 0, -LIMIT - 1, 0), (0, 0, 0, LIMIT + 2), (0, -LIMIT - 2, 0, 0),
             (15, 2, -9, 4), (-1, 2, -9, 4), (16, 2, -9, 4), (3, 2 ** 20, 0, 0), (0, 2 ** 19, 3, -5), (1, -(2 ** 19), 3, -5)]
    return np.concatenate([limit_set(), np.array(extra, np.int32), ordinary_rows(150, 9, 4, seed=106)])


def count_rows(cap):
    """exactly `cap` ordinary rows for the device-count tests, negative ones included, about 40 % of them repeats; no row is
    refused at q = 1, 2 or 4, so any status bit comes from a read of a dead row"""
    distinct = cap - int(0.4 * cap)
    rows = ordinary_rows(distinct, 24, 3, seed=cap)
    rng = np.random.default_rng(cap + 1)
    out = np.concatenate([rows, rows[rng.integers(0, distinct, cap - distinct)]])
    rng.shuffle(out)
    return out


def hash_load_rows():
    """1,023 distinct keys for a table of 1,024 slots (a few of them at the limit), and 2,000 keys that are not among them:
    1,900 in range, 100 out of range"""
    keys = np.concatenate([np.array(limit_rows()[-20:] + [(14, LIMIT, -LIMIT, LIMIT)], np.int32), ordinary_rows(1002, 8, 3, seed=108)])
    have = set(rows_of(keys))
    absent = [r for r in rows_of(ordinary_rows(2600, 12, 4, seed=109)) if r not in have][:1900]
    absent += [(i % 3, LIMIT + 1 + i, i, -i) for i in range(40)] + [(15 + i, i, 2, 3) for i in range(30)]
    absent += [(1, 5, -LIMIT - 1 - 7 * i, 5) for i in range(30)]
    return keys, np.array(absent, np.int32)


def three_key_rows(n=20000):
    """n rows over three distinct keys (one at the limit); the third key first appears far down the list"""
    keys = np.array([(0, 3, -4, 5), (14, LIMIT, -LIMIT, LIMIT - 1), (1, -1, -1, -1)], np.int32)
    rng = np.random.default_rng(110)
    pick = np.concatenate([rng.integers(0, 2, n // 4), rng.integers(0, 3, n - n // 4)])
    pick[:3] = (1, 1, 0)
    return keys[pick]


def rank_rows(stride, dims):
    """rows for the rank volume of a dims grid at `stride`: about half the cells (one row each), and rows off the grid: negative,
    not a multiple of the stride, at and past each extent"""
    rng = np.random.default_rng(107 + stride)
    gx, gy, gz = dims
    cells = [(0, x * stride, y * stride, z * stride) for x in range(gx) for y in range(gy) for z in range(gz)]
    keep = [cells[i] for i in rng.permutation(len(cells))[:len(cells) // 2]]
    keep += [(0, (gx - 1) * stride, (gy - 1) * stride, (gz - 1) * stride), (0, 0, 0, 0)]
    off = [(0, -stride, 0, 0), (0, 0, -stride, 0), (0, 0, 0, -stride), (0, -1, -1, -1),
           (0, gx * stride, 0, 0), (0, 0, gy * stride, 0), (0, 0, 0, gz * stride),
           (0, (gx + 1) * stride, stride, stride), (0, stride, (gy + 2) * stride, 0), (0, 0, stride, (gz + 3) * stride),
           # inside the other extents but past its own: a swap of two extents lets these in or throws others out
           (0, (gy - 1) * stride, 0, 0), (0, 0, (gz - 1) * stride, 0)]
    if stride > 1:
        off += [(0, 1, 0, 0), (0, 0, stride + 1, 0), (0, stride, stride, 2 * stride - 1)]
    rows = list(dict.fromkeys(keep)) + off
    order = rng.permutation(len(rows))
    return np.array([rows[i] for i in order], np.int32)
