"""Host: what oracle/grid_ops.py (pinned to the reference at D = 24 by tests/test_oracle_grid_ops.py) makes of the selection
patterns of tests/grid_cases.py, before tests/test_grid_edges_gpu.py compares the kernels with it: the row counts worked out by
hand, the strays ignored, the order of the rows irrelevant, and the raster order of the result."""
import numpy as np
import pytest

import grid_cases as G
from oracle import grid_ops as OG


def select(names, D, cell, **kw):
    logit, coords = G.voxel_list(names, D, cell, **kw)
    with np.errstate(over="ignore", invalid="ignore"):
        return OG.init_select(logit, coords, len(names), dim=D, cell=cell, thr=G.THRESHOLD)


@pytest.mark.parametrize("D", G.DIMS)
def test_row_counts_worked_out_by_hand(D):
    seen = 0
    for name in G.PATTERNS:
        want = G.expected_rows(name, D)
        for cell in G.CELLS:
            rows = select((name,), D, cell)
            if want is not None:
                assert rows.shape[0] == want, (name, D, cell)
                seen += 1
            vol = OG.dilate(OG.dilate(OG.erode(G.pattern(name, D))))
            assert np.array_equal(rows, G.raster_rows(vol, 0, cell))         # raster order, scaled by the cell
    assert seen >= 9


def test_table_of_the_issue():
    assert [G.expected_rows("full", d) for d in G.DIMS] == [0, 0, 27, 125, 13824, 29791, 32768]
    assert [G.expected_rows("corners", d) for d in G.DIMS] == [0, 0, 27, 125, 512, 512, 512]
    assert [G.expected_rows("slab", d) for d in G.DIMS] == [0, 0, 27, 100, 2304, 3844, 4096]
    assert G.expected_rows("random93", 32) == 31937 and G.expected_rows("random50", 32) == 0
    assert int(G.pattern("slab", 32)[0, 0].sum()) == 3 and G.pattern("slab", 32)[0, 0, 31]


@pytest.mark.parametrize("D,cell", [(5, 2), (32, 4), (3, 1)])
def test_batches_strays_and_order(D, cell):
    names = ("corners", "slab", "random93")
    rows = select(names, D, cell)
    parts = [select((n,), D, cell, strays=False) for n in names]
    for b, part in enumerate(parts):
        part[:, 0] = b
    assert np.array_equal(rows, np.concatenate(parts))                      # per element, in element order; strays ignored
    assert np.array_equal(rows, select(names, D, cell, seed=5))               # the order of the list does not matter
    logit, coords = G.voxel_list(names, D, cell)
    assert (coords[:, 0] == -1).sum() == D ** 3 and (coords[:, 0] == len(names)).sum() == D ** 3
    assert not np.array_equal(coords, coords[np.lexsort(coords.T[::-1])])     # shuffled
    if cell > 1:        # only the last child of a cell is above the threshold
        assert np.isnan(logit).any() and np.isposinf(logit).any() and np.isneginf(logit).any()
        with np.errstate(over="ignore", invalid="ignore"):
            above = 1.0 / (1.0 + np.exp(-logit)) > G.THRESHOLD
        inside = (coords[:, 0] >= 0) & (coords[:, 0] < len(names))
        assert (coords[above & inside][:, 1:] % cell == cell - 1).all() and above[inside].any()
