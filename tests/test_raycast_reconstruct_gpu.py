"""GPU: python -m eprecon_amd.reconstruct --preview writes one ray-cast picture of the scene so far per fragment, and changes
no byte of the saved scene."""
import os

import numpy as np
import pytest

from test_reconstruct_gpu import HEIGHT, N_FRAGMENTS, SCENE, WIDTH, write_scene

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def test_preview_writes_a_picture_per_fragment_and_leaves_the_scene_alone(tmp_path):
    pytest.importorskip("PIL")
    from PIL import Image
    from eprecon_amd import raycast, reconstruct          # noqa: F401  (the module under test; reconstruct imports it lazily)
    root = str(tmp_path / "data")
    write_scene(root)
    saved = {}
    for name, extra in (("plain", []), ("preview", ["--preview"])):
        out = str(tmp_path / name)
        assert reconstruct.main(["--data_path", root, "--out", out, "--size", str(WIDTH), str(HEIGHT)] + extra) == 0
        with open(os.path.join(out, "scene_scannet_fusion_eval_0", SCENE + ".npz"), "rb") as fh:
            saved[name] = fh.read()
    assert saved["plain"] == saved["preview"]
    assert not os.path.exists(tmp_path / "plain" / "preview")
    folder = tmp_path / "preview" / "preview" / SCENE
    assert sorted(os.listdir(folder)) == [f"{f:05d}.png" for f in range(N_FRAGMENTS)]
    for f in range(N_FRAGMENTS):
        picture = np.asarray(Image.open(folder / f"{f:05d}.png"))
        assert picture.shape == (HEIGHT, WIDTH, 3) and picture.dtype == np.uint8
        seen = (picture != 255).any(-1)
        assert seen.any(), f                                     # not all background: the camera looks at what it just fused
