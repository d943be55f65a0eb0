"""CPU: the host side of the native visualizer (disvae_amd/visualize.py, viz_helpers.py) -- loss-log reading, the dataset
background table, argument errors raised before any device work, the grid geometry of dvae_image_grid_shape (host-only C
call), GIF writing, and the new C-ABI exports (header, ctypes table, plan ops)."""
import os
import re
from collections import defaultdict

import numpy as np
import pytest
import torch
from PIL import Image, ImageSequence

from disvae_amd import _lib, Visualizer, GifTraversalsTraining
from disvae_amd import viz_helpers as VH
from disvae_amd import visualize as VZ
from disvae_amd.models.vae import init_specific_model
from disvae_amd.training import LossesLogger

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reference_names_and_defaults():
    assert VZ.GIF_FILE == "training.gif" and VZ.TRAIN_FILE == "train_losses.log" and VH.FPS_GIF == 12
    assert VZ.PLOT_NAMES == dict(generate_samples="samples.png", data_samples="data_samples.png",
                                 reconstruct="reconstruct.png", traversals="traversals.png",
                                 reconstruct_traverse="reconstruct_traverse.png", gif_traversals="posterior_traversals.gif")


def test_read_loss_from_file_last_epoch_by_suffix(tmp_path):
    log = LossesLogger(str(tmp_path / "train_losses.log"))
    for epoch in range(3):
        st = defaultdict(list)
        st["loss"].append(1.0 + epoch)
        st["recon_loss"].append(2.0)
        st["kl_loss"].append(3.0)
        # written out of suffix order, 12 dimensions (string order would put kl_loss_10 before kl_loss_2)
        for i in reversed(range(12)):
            st["kl_loss_" + str(i)].append(10.0 * epoch + i + 0.25)
        log.log(epoch, st)
    got = VH.read_loss_from_file(log.path, "kl_loss_")
    assert got == [20.0 + i + 0.25 for i in range(12)]
    assert VH.read_loss_from_file(log.path, "mi_loss_") == []


def test_background_table():
    assert [VH.get_background(d) for d in ("mnist", "fashion", "dsprites", "celeba", "chairs")] == [0, 0, 0, 1, 1]
    assert VH.get_background("CelebA") == 1
    with pytest.raises(ValueError):
        VH.get_background("imagenet")
    model = init_specific_model("Burgess", (1, 32, 32), 4)
    with pytest.raises(ValueError):
        Visualizer(model, "no_such_dataset", "/nonexistent")
    assert Visualizer(model, "celeba", "/nonexistent").pad_value == 0
    assert Visualizer(model, "mnist", "/nonexistent").pad_value == 1


def test_upsample_factor_must_be_an_integer():
    model = init_specific_model("Burgess", (1, 32, 32), 4)
    for bad in (1.5, 2.0, 0, -1, True, "2"):
        with pytest.raises(ValueError):
            Visualizer(model, "mnist", "/nonexistent", upsample_factor=bad)
    assert Visualizer(model, "mnist", "/nonexistent", upsample_factor=np.int64(3)).upsample_factor == 3
    with pytest.raises(ValueError):
        GifTraversalsTraining(model, "mnist", "/nonexistent", upsample_factor=0.5)


def test_size_errors_come_before_any_device_work(tmp_path):
    model = init_specific_model("Burgess", (1, 32, 32), 4)             # on the CPU: a device pass would raise DvaeHipError
    vis = Visualizer(model, "mnist", str(tmp_path))
    with pytest.raises(ValueError, match="even number of rows"):
        vis.reconstruct(torch.rand(16, 1, 32, 32), size=(3, 4))
    with pytest.raises(ValueError, match="Wrong size"):
        vis._save_or_return(torch.rand(5, 1, 32, 32), (2, 2), "x.png")
    with pytest.raises(ValueError, match="same posterior"):
        vis.traversals(data=torch.rand(2, 1, 32, 32))
    with pytest.raises(ValueError, match="C = 1 or 3"):
        VH.image_grid_u8(torch.rand(4, 2, 8, 8))
    with pytest.raises(_lib.DvaeHipError):
        vis.generate_samples(size=(2, 2))


def test_grid_shape_is_make_grids_geometry():
    def ref(n, H, W, nrow, padding, f):
        if n == 1:
            return H * f, W * f
        xm = min(nrow, n)
        ym = -(-n // xm)
        return ym * (H * f + padding) + padding, xm * (W * f + padding) + padding
    for n in (1, 2, 7, 64, 100):
        for nrow in (1, 8, 10):
            for H, W in ((32, 32), (64, 64), (5, 9)):
                for f in (1, 2, 3):
                    for padding in (0, 2):
                        assert VH.grid_shape(n, H, W, nrow, padding, f) == ref(n, H, W, nrow, padding, f)
    assert VH.grid_shape(100, 64, 64, 10) == (662, 662)
    with pytest.raises(_lib.DvaeHipError):
        VH.grid_shape(0, 64, 64, 8)
    with pytest.raises(_lib.DvaeHipError):
        VH.grid_shape(4, 64, 64, 8, 2, 0)


def test_concatenate_pad_and_grey_gif_round_trip(tmp_path):
    a = np.full((3, 2, 3), 7, np.uint8)
    b = np.full((3, 2, 3), 9, np.uint8)
    c = VH.concatenate_pad([a, b], pad_size=2, pad_values=255, axis=1)
    assert c.dtype == np.uint8 and c.shape == (3, 12, 3)                 # pad a pad b pad pad (the reference's layout)
    assert (c[:, :2] == 255).all() and (c[:, 2:4] == 7).all() and (c[:, 4:6] == 255).all() and (c[:, 6:8] == 9).all()
    assert (c[:, 8:] == 255).all()
    rng = np.random.default_rng(0)
    frames = [np.repeat(rng.integers(0, 256, (20, 30, 1), dtype=np.uint8), 3, axis=2) for _ in range(3)]
    path = str(tmp_path / "t.gif")
    VH.save_gif(path, frames)
    im = Image.open(path)
    back = [np.asarray(f.convert("RGB")) for f in ImageSequence.Iterator(im)]
    assert len(back) == 3 and all(np.array_equal(x, y) for x, y in zip(back, frames))
    # (GIF stores delays in hundredths of a second: 83 ms reads back as 80)
    assert abs(im.info.get("duration") - round(1000 / VH.FPS_GIF)) < 10 and im.info.get("loop") == 0


def test_grid_entry_points_are_exported_and_replayable():
    hdr = open(os.path.join(ROOT, "include", "dvae_hip.h")).read()
    h = _lib.lib()
    for name in ("dvae_image_grid_u8", "dvae_image_grid_shape"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES
        assert hasattr(h, name)
        assert h.dvae_plan_op(name.encode()) >= 0, name
    assert h.dvae_version() == 109
    # argument checks fire before any launch (no GPU needed)
    with pytest.raises(_lib.DvaeHipError, match="invalid argument"):
        _lib.call("dvae_image_grid_u8", None, 4, 3, 8, 8, 2, 2, 0.0, 1, None, None)
    with pytest.raises(_lib.DvaeHipError, match="invalid argument"):
        _lib.call("dvae_image_grid_u8", 16, 4, 2, 8, 8, 2, 2, 0.0, 1, 16, None)        # C = 2
