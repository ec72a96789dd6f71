"""CPU: sparse.IdentityCache, the one cache behind modules.voxel_set_for and torchsparse_utils.VOXELIZATIONS — a hit needs the
same tensor OBJECT with the same data_ptr, version counter, row count and extra; the newest `max` entries stay, oldest first."""
import pytest

torch = pytest.importorskip("torch")
from eprecon_amd.sparse import IdentityCache  # noqa: E402


def test_hit_needs_the_same_object_pointer_version_rows_and_extra():
    cache = IdentityCache(4)
    t = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    assert cache.get(t, 0.5) is None
    cache.put((t, 0.5, "entry"))
    assert cache.get(t, 0.5) == "entry"
    assert cache.get(t, 0.25) is None and cache.get(t) is None           # another extra
    assert cache.get(t.clone(), 0.5) is None                             # equal values, another object and pointer
    assert cache.get(t[:], 0.5) is None                                  # the same pointer, version and rows: another object
    t.add_(1)                                                            # in place: the version counter moved
    assert cache.get(t, 0.5) is None
    cache.put((t, 0.5, "again"))
    assert cache.get(t, 0.5) == "again"
    t.set_(torch.zeros(3, 4))                                            # the same object on other storage
    assert cache.get(t, 0.5) is None


def test_row_count_is_part_of_the_key():
    cache = IdentityCache(4)
    t = torch.zeros(6, 4)
    cache.put((t, None, "six rows"))
    version, ptr = t._version, t.data_ptr()
    with torch.autograd._unsafe_preserve_version_counter(t):            # (what a write through raw pointers looks like)
        t.resize_(3, 4)                                                  # shrinks in its storage: the pointer stays
    assert (t._version, t.data_ptr()) == (version, ptr)
    assert cache.get(t) is None


def test_keeps_the_newest_entries_in_fifo_order():
    cache = IdentityCache(3)
    ts = [torch.zeros(2, 4) for _ in range(6)]
    for i in range(3):
        cache.put((ts[i], 1, i))
    assert cache.values() == [0, 1, 2]
    cache.put((ts[3], 1, 3))
    assert cache.values() == [1, 2, 3] and cache.get(ts[0], 1) is None and cache.get(ts[1], 1) == 1
    cache.put((ts[4], 1, 4), (ts[5], 1, 5))                              # two at once: the two oldest leave
    assert cache.values() == [3, 4, 5]
    assert [cache.get(t, 1) for t in ts] == [None, None, None, 3, 4, 5]
    cache.put(*((ts[i], 2, 10 + i) for i in range(5)))                   # more than the bound at once: its newest `max`
    assert cache.values() == [12, 13, 14]


def test_clear_empties_it():
    cache = IdentityCache(2)
    t = torch.zeros(1, 4)
    cache.put((t, 1, "x"))
    cache.clear()
    assert cache.values() == [] and cache.get(t, 1) is None


def test_the_package_caches_keep_their_bounds_and_clear_together():
    from eprecon_amd import modules as M
    from eprecon_amd import torchsparse_utils as TU
    coords = [torch.zeros((2, 4), dtype=torch.int32) for _ in range(10)]
    M.clear_coordinate_caches()
    sets = [M.voxel_set_for(c) for c in coords]
    assert M.voxel_set_for(coords[-1]) is sets[-1] and M.voxel_set_for(coords[2]) is sets[2]     # the newest 8 of 10
    assert M.voxel_set_for(coords[1]) is not sets[1]
    TU.VOXELIZATIONS.put(*((c, 1.0, i) for i, c in enumerate(coords)))
    assert TU.VOXELIZATIONS.values() == [4, 5, 6, 7, 8, 9]                                       # the newest 6 of 10
    M.clear_coordinate_caches()
    assert TU.VOXELIZATIONS.values() == [] and M.voxel_set_for(coords[-1]) is not sets[-1]
    M.clear_voxel_set_cache()
