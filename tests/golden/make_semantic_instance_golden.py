"""Writes tests/golden/semantic_instance.npz from the reference's own tools/generate_semantic_instance.py, run in place on a
seeded scene.  Build container only.

    python tests/golden/make_semantic_instance_golden.py

The reference's file is loaded by path with an empty stand-in for `plyfile` in sys.modules and its `read_ply` replaced by a
function that returns the fixture's vertices (its mesh directory is hard-wired); it reads
results/scene_scannet_checkpoints_fusion_eval_99/<scene>.npz and writes semantic/ and instance/ relative to the working
directory, so it runs inside a temporary one.

Recorded: the inputs (semantic, instance, origin, voxel_size, vertices), the reference's per-vertex semantic ids, its
instance lines and masks, and the raw bytes of its three kinds of text file.  Data only.

Checked before anything is written (the file is not written otherwise):
  * no vertex has a second-nearest site within a relative 1e-9 of the nearest in d2 (the two tie rules cannot differ);
  * the float64 brute force of tests/label_transfer_ref.py gives the reference's semantic id for every vertex, and its
    instance ids give the reference's masks;
  * there are vertices outside the volume on all six sides, and vertices further from every site than two brick shells.
"""
import glob
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_shim  # noqa: E402
import label_transfer_ref as R  # noqa: E402

SCENE = "s0"
DIMS = (13, 10, 7)                     # no axis a multiple of the brick edge
ORIGIN = np.array([-1.23, 0.57, 2.01], np.float32)
VOXEL_SIZE = np.float64(0.04)
INSTANCE_IDS = np.array([0, 7, 14, 21, 28])
N_VERTS, GROW = 3000, 0.3


def inputs():
    rng = np.random.default_rng(20241019)
    sem = np.zeros(DIMS, np.int32)
    ins = np.zeros(DIMS, np.int32)
    for sl in ((slice(0, 4), slice(0, 5), slice(0, 4)), (slice(7, 11), slice(5, 10), slice(2, 7))):     # two blobs, empty middle
        shape = sem[sl].shape
        sem[sl] = rng.integers(0, 21, shape)
        ins[sl] = rng.choice(INSTANCE_IDS, shape)
    sem[12, 9, 6], ins[12, 9, 6] = 5, 14                  # one labelled cell at the far corner
    lo = ORIGIN.astype(np.float64) - GROW
    hi = ORIGIN.astype(np.float64) + (np.array(DIMS) - 1) * float(VOXEL_SIZE) + GROW
    verts = (lo + rng.random((N_VERTS, 3)) * (hi - lo)).astype(np.float32)
    return sem, ins, verts


def run_reference(sem, ins, verts):
    sys.modules.setdefault("plyfile", types.ModuleType("plyfile"))
    spec = importlib.util.spec_from_file_location("ref_generate_semantic_instance",
                                                  os.path.join(ref_shim.REF, "tools", "generate_semantic_instance.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.read_ply = lambda path: verts
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        d = os.path.join(tmp, "results", "scene_scannet_checkpoints_fusion_eval_99")
        os.makedirs(d)
        np.savez(os.path.join(d, SCENE + ".npz"), origin=ORIGIN, voxel_size=VOXEL_SIZE, tsdf=np.ones(DIMS, np.float32),
                 semantic=sem, instance=ins)
        os.chdir(tmp)
        try:
            mod.generate_semantic_instance(SCENE)
        finally:
            os.chdir(cwd)
        read = lambda *p: open(os.path.join(tmp, *p), "rb").read()
        masks = sorted(glob.glob(os.path.join(tmp, "instance", "predicted_masks", SCENE + "_*.txt")))
        return read("semantic", SCENE + ".txt"), read("instance", SCENE + ".txt"), [open(m, "rb").read() for m in masks]


def main():
    sem, ins, verts = inputs()
    sem_txt, ins_txt, mask_txts = run_reference(sem, ins, verts)
    ref_sem = np.array(sem_txt.split(), np.int64)
    ref_masks = np.stack([np.array(m.split(), np.uint8) for m in mask_txts])
    lines = ins_txt.decode("ascii").splitlines()
    bf = R.brute_force(sem, ins, ORIGIN, VOXEL_SIZE, verts)

    ambiguous = int((bf["second"] <= bf["d2"] * (1.0 + 1e-9)).sum())
    equal = int((bf["semantic"] == ref_sem).sum())
    ids = np.unique(bf["instance"])
    print(f"ambiguous {ambiguous} of {N_VERTS}; semantic equal {equal} of {N_VERTS}; instances {len(ids)}")
    assert ambiguous == 0
    assert equal == N_VERTS and ref_sem.shape == (N_VERTS,)
    assert ref_masks.shape == (len(ids), N_VERTS) and all((ref_masks[i] == (bf["instance"] == k)).all() for i, k in enumerate(ids))
    assert len(lines) == len(ids) == len(INSTANCE_IDS)
    box_lo = ORIGIN.astype(np.float64)
    box_hi = box_lo + (np.array(DIMS) - 1) * float(VOXEL_SIZE)
    assert (verts < box_lo).any(0).all() and (verts > box_hi).any(0).all()        # outside on all six sides
    far = float(bf["dist"].max() / VOXEL_SIZE)
    print(f"farthest vertex: {far:.1f} cells from its site")
    assert far > 12.0                                                              # beyond two shells of 4-cell bricks

    out = os.path.join(HERE, "semantic_instance.npz")
    np.savez_compressed(out, semantic=sem, instance=ins, origin=ORIGIN, voxel_size=VOXEL_SIZE, vertices=verts,
                        ref_semantic=ref_sem.astype(np.int32), ref_masks=ref_masks,
                        ref_instance_class=np.array([int(l.split()[1]) for l in lines], np.int32),
                        semantic_txt=np.frombuffer(sem_txt, np.uint8), instance_txt=np.frombuffer(ins_txt, np.uint8),
                        mask_txt=np.stack([np.frombuffer(m, np.uint8) for m in mask_txts]))
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
