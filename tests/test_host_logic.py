"""CPU: host-side logic of the native package (no kernels): API surface, parameter arena,
state_dict compatibility, annealing / storer cadence, log importance weights."""
import math
import os
import sys
from collections import defaultdict

import numpy as np
import pytest
import torch

from oracle import disvae_oracle as O
from golden_util import load
import disvae_amd
from disvae_amd.models import losses as L
from disvae_amd.models.vae import init_specific_model, VAE, MODELS
from disvae_amd.models.discriminator import Discriminator
from disvae_amd.utils.math import log_importance_weights


def test_api_surface():
    assert L.LOSSES == O.LOSSES == ["VAE", "betaH", "betaB", "factor", "btcvae"]
    assert L.RECON_DIST == O.RECON_DIST and MODELS == ["Burgess"]
    assert hasattr(disvae_amd, "Trainer") and hasattr(disvae_amd, "init_specific_model")
    with pytest.raises(ValueError):
        init_specific_model("Foo", (1, 32, 32), 10)
    with pytest.raises(RuntimeError):
        init_specific_model("Burgess", (1, 28, 28), 10)
    with pytest.raises(ValueError):
        L.get_loss_f("nope", rec_dist="bernoulli", reg_anneal=0)
    kw = dict(rec_dist="bernoulli", reg_anneal=10000, betaH_B=4, betaB_initC=0, betaB_finC=25, betaB_G=1000,
              factor_G=6.4, latent_dim=10, lr_disc=1e-4, btcvae_A=1, btcvae_B=6.4, btcvae_G=1, n_data=100,
              device=torch.device("cpu"))
    assert isinstance(L.get_loss_f("VAE", **kw), L.BetaHLoss) and L.get_loss_f("VAE", **kw).beta == 1
    assert L.get_loss_f("betaH", **kw).beta == 4
    b = L.get_loss_f("betaB", **kw)
    assert (b.C_init, b.C_fin, b.gamma) == (0, 25, 1000)
    t = L.get_loss_f("btcvae", **kw)
    assert (t.n_data, t.alpha, t.beta, t.gamma, t.is_mss) == (100, 1, 6.4, 1, True)
    f = L.get_loss_f("factor", **kw)
    assert f.gamma == 6.4 and f.optimizer_d.defaults["betas"] == (0.5, 0.9) and f.optimizer_d.defaults["lr"] == 1e-4
    with pytest.raises(ValueError):          # control-flow exception of losses.py:240-241
        f(None, None, None, True, None)


@pytest.mark.parametrize("img", [(1, 32, 32), (1, 64, 64), (3, 64, 64)])
def test_same_seed_same_weights_and_state_dict(img):
    torch.manual_seed(1234)
    m = init_specific_model("Burgess", img, 10)
    torch.manual_seed(1234)
    ref = O.init_vae_params(img, 10)
    sd = m.state_dict()
    assert list(sd.keys()) == list(ref.keys())
    for k in ref:
        assert sd[k].shape == ref[k].shape and torch.equal(sd[k], ref[k]), k
    n = sum(p.numel() for p in m.parameters())
    assert n == {(1, 32, 32): 469173, (1, 64, 64): 502005, (3, 64, 64): 504055}[img]   # SURVEY 2b [probe]
    # parameters are views into ONE flat arena; load_state_dict writes through
    new = {k: torch.full_like(v, 0.5) for k, v in ref.items()}
    m.load_state_dict(new)
    assert float(m.arena.flat[:10].mean()) == 0.5
    assert m.encoder.conv1.weight.data_ptr() == m.arena.flat.data_ptr()
    m.assign_grads()
    assert m.encoder.conv1.weight.grad.data_ptr() == m.arena.grad.data_ptr()


def test_discriminator_init_matches():
    torch.manual_seed(3)
    d = Discriminator(latent_dim=10)
    torch.manual_seed(3)
    ref = O.init_disc_params(10)
    assert sum(p.numel() for p in d.parameters()) == 4017002
    for k, v in d.state_dict().items():
        assert torch.equal(v, ref[k]), k


def test_annealing_and_storer_cadence():
    assert L.linear_annealing(0, 1, 1, 10000) == 1e-4
    assert L.linear_annealing(0, 25, 5000, 100000) == 1.25
    assert L.linear_annealing(0, 1, 99, 0) == 1
    assert L.linear_annealing(0, 1, 20000, 10000) == 1
    with pytest.raises(AssertionError):
        L.linear_annealing(1, 1, 1, 10)
    lf = L.BetaHLoss(beta=4, rec_dist="bernoulli", steps_anneal=10)
    kept = []
    for i in range(1, 103):
        s = lf._pre_call(True, defaultdict(list))
        kept.append(s is not None)
    assert [i + 1 for i, k in enumerate(kept) if k] == [1, 51, 101] and lf.n_train_steps == 102
    assert lf._pre_call(False, {}) is not None and lf.n_train_steps == 102     # eval keeps the storer


def test_log_importance_weights_match_matrix():
    g = load("kats")
    for (b, n) in [(4, 100), (8, 737280), (64, 202599)]:
        W = g["kat_logiw_%d_%d" % (b, n)]
        lw = log_importance_weights(b, n).numpy()
        assert W[0, 0] == lw[0] and W[0, 1] == lw[1] and W[0, 2] == lw[2]
        assert W[b - 2, 0] == lw[1]                       # the W[M-1, 0] exception cell
        expect = np.full((b, b), lw[2], dtype=np.float32)
        expect[:, 0] = lw[0]; expect[:, 1] = lw[1]; expect[b - 2, 0] = lw[1]
        np.testing.assert_array_equal(W, expect)


def test_checkpoint_roundtrip(tmp_path):
    from disvae_amd.utils.modelIO import save_model, load_model, load_metadata
    torch.manual_seed(0)
    m = init_specific_model("Burgess", (1, 32, 32), 10)
    save_model(m, str(tmp_path))
    meta = load_metadata(str(tmp_path))
    assert meta["model_type"] == "Burgess" and meta["latent_dim"] == 10
    m2 = load_model(str(tmp_path), is_gpu=False)
    for (k1, v1), (k2, v2) in zip(m.state_dict().items(), m2.state_dict().items()):
        assert k1 == k2 and torch.equal(v1, v2)
    assert not m2.training


def test_launch_plan_record_and_replay_order():
    """graph.StepGraphs mode "plan": the first call with a key executes AND records, later calls with the same key
    re-issue the recorded entries in order without running the step function; a new key records again
    (host logic only: python callables stand in for the C-ABI launches)."""
    from disvae_amd import _lib
    from disvae_amd.graph import StepGraphs
    log = []
    runs = []

    def step(tag):
        runs.append(tag)
        _lib.record_py(log.append, (tag, "fork"))
        _lib.record_py(log.append, (tag, "kernel-1"))
        _lib.record_py(log.append, (tag, "kernel-2"))

    g = StepGraphs()
    g.run(("k", 1), lambda: step("a"), "plan")            # records while executing
    assert runs == ["a"] and log == [("a", "fork"), ("a", "kernel-1"), ("a", "kernel-2")]
    g.run(("k", 1), lambda: step("never"), "plan")        # replay: the step function is not called
    assert runs == ["a"] and log[3:] == [("a", "fork"), ("a", "kernel-1"), ("a", "kernel-2")]
    assert g.replays == 1
    g.run(("k", 2), lambda: step("b"), "plan")            # other key (e.g. another batch pointer): new plan
    assert runs == ["a", "b"] and g.replays == 1
    assert _lib._REC is None                              # recording always ends, also on the error path:
    try:
        g.run(("k", 3), lambda: 1 / 0, "plan")
    except ZeroDivisionError:
        pass
    assert _lib._REC is None


def test_allocation_generation_invalidates_plan_keys():
    """Every (re)allocation of engine buffers bumps _lib.ALLOC_GEN; the loss plugins put it into their plan key, so a
    plan holding stale pointers can never be replayed."""
    from disvae_amd import _lib
    g0 = _lib.ALLOC_GEN[0]
    _lib.note_alloc()
    assert _lib.ALLOC_GEN[0] == g0 + 1


REF_CHECKPOINTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_checkpoints.npz")


def _reference_checkpoint(name, d):
    """results/<name>/ as the reference wrote it (recorded by tests/golden/make_golden.py --checkpoints): specs.json verbatim,
    model.pt = the reference's file (torch's legacy serialisation: its pickled header, then per storage an int64 element
    count and the raw fp32 values) with seeded values in place of the trained weights."""
    import numpy as np
    g = np.load(REF_CHECKPOINTS)
    with open(os.path.join(d, "specs.json"), "wb") as f:
        f.write(g[name + "_specs"].tobytes())
    rng = np.random.default_rng(1234)
    with open(os.path.join(d, "model.pt"), "wb") as f:
        f.write(g[name + "_header"].tobytes())
        for n in g[name + "_numel"]:
            f.write(np.array(n, dtype="<i8").tobytes())
            f.write(rng.standard_normal(int(n), dtype=np.float32).astype("<f4").tobytes())


@pytest.mark.parametrize("name", ["btcvae_dsprites", "factor_celeba", "VAE_mnist"])
def test_reference_checkpoints_load_into_the_native_model(name, tmp_path):
    """results/*/model.pt + specs.json written by the reference load through the native
    load_model (modelIO.py:81-153) -- same state_dict keys / shapes, every tensor bit-identical, weights land in the
    flat parameter arena that the HIP engine reads."""
    from disvae_amd.utils.modelIO import load_model, load_metadata
    d = str(tmp_path)
    _reference_checkpoint(name, d)
    meta = load_metadata(d)
    model = load_model(d, is_gpu=False)
    state = torch.load(os.path.join(d, "model.pt"), map_location="cpu")
    own = model.state_dict()
    assert list(own.keys()) == list(state.keys())
    for k, v in state.items():
        assert own[k].shape == v.shape and torch.equal(own[k], v), k
    assert tuple(model.img_size) == tuple(meta["img_size"]) and model.latent_dim == meta["latent_dim"]
    # the parameters ARE views of the arena
    w = model.encoder.conv1.weight
    assert w.data_ptr() == model.arena.view("encoder.conv1.weight").data_ptr()
    assert not model.training


def test_bench_algorithmic_flops_match_survey():
    """bench.py's step_tflops / roofline figures are computed from SURVEY 8d's algorithmic FLOPs per image
    (6 MACs_fwd - 2 MACs_conv1): 84.19 MFLOP at 64x64x3, 73.71 MFLOP at 64x64x1; the dominant kernel's launch
    (conv2 forward, 1024 images) is 8.59 GFLOP."""
    import importlib
    bench = importlib.import_module("bench")
    assert abs(bench.flops_per_image_train(3) / 1e6 - 84.19) < 0.01
    assert abs(bench.flops_per_image_train(1) / 1e6 - 73.71) < 0.01
    assert abs(2.0 * 4194304 * 1024 / 1e9 - 8.59) < 0.01
    assert bench.PEAK_FP32_MFMA_TFLOPS == 157.3 and bench.PEAK_HBM_GBS == 8000.0


def test_latent_dim_limits_are_reported_clearly():
    """a latent dimension the model cannot have must fail at construction with a clear message, not with a generic
    'bad argument' from the C-ABI at the first training step.  (Round 5: every positive integer is a valid dimension --
    test_any_latent_dim_is_accepted_for_every_loss; what remains to refuse is what is not one.)"""
    import pytest
    from disvae_amd.models.vae import init_specific_model
    for D in (1, 10, 16, 17, 64):
        assert init_specific_model("Burgess", (1, 32, 32), D).latent_dim == D
    for D in (0, -3, 10.0):
        with pytest.raises(ValueError, match="latent_dim"):
            init_specific_model("Burgess", (1, 32, 32), D)


def test_unknown_replay_mode_is_reported(monkeypatch):
    import pytest
    from disvae_amd.models.losses import BetaHLoss
    monkeypatch.setenv("DVAE_REPLAY", "sometimes")
    assert BetaHLoss().replay == "auto"          # host A/B switches are inert without DVAE_DEBUG=1 (disvae_amd/_debug.py)
    monkeypatch.setenv("DVAE_DEBUG", "1")
    with pytest.raises(ValueError, match="DVAE_REPLAY"):
        BetaHLoss()
    monkeypatch.setenv("DVAE_REPLAY", "eager")
    assert BetaHLoss().replay is None


def test_bench_reads_hbm_traffic_from_the_newest_pmc_summary(tmp_path, monkeypatch):
    """roofline traffic comes from the newest committed PMC summary THAT HAS THE ROW of the exact template variant: within a
    round the `_final_` summary is newer than any `_runN_` one, a later round beats an earlier one; value = fetch MB + write MB
    of that variant (no averaging over the plain / masked variants of a family)."""
    import importlib
    bench = importlib.import_module("bench")
    prof = tmp_path / "profiles"
    prof.mkdir()
    head = "| kernel | A | fetch MB (x2 corr) | write MB | mfma_busy/gui |\n|---|---|---|---|---|\n"
    (prof / "r02_run6_pmc_summary.md").write_text(head + "| k_up32ws<16, true> | 1 | 100.0 | 50.0 | 0.5 |\n")
    (prof / "r02_final_pmc_summary.md").write_text(head + "| k_up32ws<16, true> | 1 | 180.0 | 130.0 | 0.5 |\n"
                                                          "| k_up32ws<16, false> | 1 | 50.0 | 130.0 | 0.6 |\n")
    (prof / "r01_run31_pmc_summary.md").write_text(head + "| k_up32ws<16, true> | 1 | 1.0 | 1.0 | 0.5 |\n")
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    bytes_, src, ipl = bench.pmc_traffic("k_up32ws<16, true>", 1024)
    assert src == os.path.join("profiles", "r02_final_pmc_summary.md") and ipl == 1024
    assert abs(bytes_ - 310.0e6) < 1.0
    assert abs(bench.pmc_traffic("k_up32ws<16, false>", 1024)[0] - 180.0e6) < 1.0
    (prof / "r03_run1_pmc_summary.md").write_text(head + "| k_up32ws<16, true> | 1 | 170.0 | 130.0 | 0.5 |\n")
    assert bench.pmc_traffic("k_up32ws<16, true>", 1024)[1] == os.path.join("profiles", "r03_run1_pmc_summary.md")
    # a variant the newest summary does not list falls back to the newest one that does
    assert bench.pmc_traffic("k_up32ws<16, false>", 1024)[1] == os.path.join("profiles", "r02_final_pmc_summary.md")
    assert bench.pmc_traffic("k_up32ws<16", 1024) == (None, None, None)           # a prefix is not a row
    assert bench.pmc_traffic("k_no_such_kernel", 1024) == (None, None, None)
    # a numbered final visit beats every vNN / runNN visit of its round whatever the numbers (round 4: r04_v35 was picked
    # over r04_final3), a later numbered final beats an earlier one, the next round's first visit beats them all
    (prof / "r04_v35_pmc_summary.md").write_text(head + "| k_up_thin_pk<3, true, float> | 1 | 240.0 | 104.3 | 0.0 |\n")
    (prof / "r04_final3_pmc_summary.md").write_text(head + "| k_up_thin_pk<3, true, float> | 1 | 186.3 | 100.7 | 0.0 |\n")
    (prof / "r04_final2_pmc_summary.md").write_text(head + "| k_up_thin_pk<3, true, float> | 1 | 200.0 | 100.0 | 0.0 |\n")
    bytes_, src, _ = bench.pmc_traffic("k_up_thin_pk<3, true, float>", 1024)
    assert src == os.path.join("profiles", "r04_final3_pmc_summary.md") and abs(bytes_ - 287.0e6) < 1.0
    (prof / "r05_v2_pmc_summary.md").write_text(head + "| k_up_thin_pk<3, true, float> | 1 | 190.0 | 100.0 | 0.0 |\n")
    assert bench.pmc_traffic("k_up_thin_pk<3, true, float>", 1024)[1] == os.path.join("profiles", "r05_v2_pmc_summary.md")
    # images per launch: a summary collected AT the asked size wins over a newer one collected elsewhere; otherwise the newest
    # is scaled by images / its own size; FactorVAE summaries without a header (means over mixed launch sizes) are never used
    (prof / "r06_v1_b128_pmc_summary.md").write_text("images_per_launch: 128  (x)\n\n" + head + "| k_down_thin<3, 3, float> | 1 | 6.0 | 17.6 | 0.0 |\n")
    (prof / "r06_v2_pmc_summary.md").write_text("images_per_launch: 1024\n\n" + head + "| k_down_thin<3, 3, float> | 1 | 50.0 | 140.0 | 0.0 |\n")
    (prof / "r06_v3_factor_pmc_summary.md").write_text(head + "| k_down_thin<3, 3, float> | 1 | 99.0 | 300.0 | 0.0 |\n"
                                                              "| k_only_in_factor | 1 | 1.0 | 1.0 | 0.0 |\n")
    bytes_, src, ipl = bench.pmc_traffic("k_down_thin<3, 3, float>", 128)
    assert src == os.path.join("profiles", "r06_v1_b128_pmc_summary.md") and ipl == 128 and abs(bytes_ - 23.6e6) < 1.0
    bytes_, src, ipl = bench.pmc_traffic("k_down_thin<3, 3, float>", 256)
    assert src == os.path.join("profiles", "r06_v2_pmc_summary.md") and ipl == 1024 and abs(bytes_ - 190.0e6 / 4) < 1.0
    assert bench.pmc_traffic("k_only_in_factor", 1024) == (None, None, None)
    assert bench.pmc_images_per_launch(str(prof / "r05_v2_pmc_summary.md")) == 1024
    assert bench.pmc_images_per_launch(str(prof / "r06_v3_factor_pmc_summary.md")) is None
    names = ["r02_run6_x.md", "r02_final_x.md", "r03_run1_x.md", "r04_v35_x.md", "r04_final_x.md", "r04_final2_x.md", "r05_v1_x.md"]
    assert sorted(reversed(names), key=bench.pmc_file_order) == names


def test_device_image_loader_draws_batches_like_the_reference_dataloader():
    """DeviceImageLoader(shuffle=True) == DataLoader(dataset, batch_size, shuffle=True) (utils/datasets.py:67-71) for the
    same torch.manual_seed: same images per batch, same ragged last batch, same state of the CPU generator afterwards;
    under data parallelism the ranks partition each global batch in rank order and agree on the number of batches."""
    from torch.utils.data import DataLoader, TensorDataset
    from disvae_amd.data import DeviceImageLoader
    n, B = 37, 8
    imgs = (torch.arange(n, dtype=torch.uint8).view(n, 1, 1, 1) * torch.ones(1, 1, 4, 4, dtype=torch.uint8)).contiguous()
    labels = torch.arange(n)
    for epoch_seed in (0, 1234):
        torch.manual_seed(epoch_seed)
        ref = [(x[:, 0, 0, 0].tolist(), y.tolist()) for x, y in DataLoader(TensorDataset(imgs, labels), batch_size=B, shuffle=True)]
        ref_next = torch.rand(3)
        torch.manual_seed(epoch_seed)
        got = [(x[:, 0, 0, 0].tolist(), y.tolist()) for x, y in DeviceImageLoader(imgs, batch_size=B, labels=labels, device="cpu")]
        assert got == ref and torch.equal(torch.rand(3), ref_next)
    # two ranks: every global batch of 2 x 4 images is the reference's batch of 8, split in rank order
    shards = []
    for rank in range(2):
        torch.manual_seed(1234)
        ld = DeviceImageLoader(imgs, batch_size=4, labels=labels, device="cpu", rank=rank, world_size=2)
        shards.append([x[:, 0, 0, 0].tolist() for x, _ in ld])
        assert len(ld) == len(shards[-1]) == 5
    for k in range(4):
        assert shards[0][k] + shards[1][k] == ref[k][0]
    assert shards[0][4] + shards[1][4] == ref[4][0][:2] + ref[4][0][2:4]       # 5 leftover images: 2 + 2, one dropped
    # no shuffle: slices in order
    ld = DeviceImageLoader(imgs, batch_size=10, shuffle=False, device="cpu")
    assert [x.shape[0] for x, _ in ld] == [10, 10, 10, 7]


# ---------------------------------------------------------------------------------- bench.py host logic (no GPU)
def _bench_module():
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(root, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    argv, sys.argv = sys.argv, ["bench.py"]
    try:
        spec.loader.exec_module(mod)
    finally:
        sys.argv = argv
    return mod


def test_bench_refuses_without_gpu_and_names_the_reason():
    """no CPU fallback: the benchmark exits with a clear message instead of timing the oracle (tier rule 3)"""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if torch.cuda.is_available():
        pytest.skip("needs a box without a GPU")
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "1", "--warmup", "0"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode != 0
    assert "no CPU fallback" in (r.stdout + r.stderr)


def test_bench_workloads_are_the_baseline_configs():
    """the five workloads of BASELINE.json (configs[0..4]) by shape, batch, loss and n_data"""
    import json
    b = _bench_module()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    base = json.load(open(os.path.join(root, "BASELINE.json")))
    assert set(b.CONFIGS) == {"vae_mnist", "btcvae_celeba", "factor_celeba", "btcvae_dsprites", "factor_dsprites"}
    assert sorted(c["baseline_config"] for c in b.CONFIGS.values()) == list(range(len(base["configs"])))
    for name, cfg in b.CONFIGS.items():
        if name == "vae_mnist":                  # configs[0]: the reference's CPU-runnable plumbing case
            assert tuple(cfg["img"]) == (1, 32, 32) and cfg["loss"] == "VAE" and cfg["batch"] == 64 and cfg["baseline_config"] == 0
            continue
        assert tuple(cfg["img"]) == ((3, 64, 64) if "celeba" in name else (1, 64, 64))
        assert cfg["loss"] == name.split("_")[0]
        assert cfg["n_data"] == (202599 if "celeba" in name else 737280)
        assert 1 <= cfg["baseline_config"] < len(base["configs"])
    assert b.CONFIGS["btcvae_celeba"]["batch"] == 1024 and b.CONFIGS["factor_celeba"]["batch"] == 2048
    assert b.CONFIGS["btcvae_dsprites"]["batch"] == 256 and b.CONFIGS["factor_dsprites"]["batch"] == 256


def test_bench_pmc_traffic_parser(tmp_path, monkeypatch):
    """`traffic` of the roofline entries = FETCH + WRITE megabytes of the newest committed PMC summary, per template variant"""
    b = _bench_module()
    prof = tmp_path / "profiles"
    prof.mkdir()
    hdr = "| kernel | A | FETCH_MB | WRITE_MB | mfma_busy |\n|---|---|---|---|---|\n"
    (prof / "r02_final_pmc_summary.md").write_text(hdr + "| k_down32dma<16, false> | 1 | 100.0 | 20.0 | 0.5 |\n")
    (prof / "r03_final_pmc_summary.md").write_text(hdr + "| k_down32dma<16, false> | 1 | 160.0 | 33.6 | 0.6 |\n"
                                                   "| k_down32dma<16, true> | 1 | 193.6 | 33.6 | 0.5 |\n")
    monkeypatch.setattr(b, "ROOT", str(tmp_path))
    val, src, ipl = b.pmc_traffic("k_down32dma<16, false>", 1024)
    assert src.endswith("r03_final_pmc_summary.md") and ipl == 1024
    assert abs(val - (160.0 + 33.6) * 1e6) < 1.0
    assert abs(b.pmc_traffic("k_down32dma<16, true>", 512)[0] - (193.6 + 33.6) * 1e6 / 2) < 1.0
    assert b.pmc_traffic("k_nonexistent", 1024) == (None, None, None)


def test_bench_starts_its_own_ranks_for_gpus_above_one(monkeypatch):
    """`python bench.py --gpus N` without a launcher re-executes itself under torch.distributed.run (VERDICT r5 missing #2): the
    command line, and that the JSON line of rank 0 stays the last line of stdout."""
    import io
    import subprocess
    b = _bench_module()
    cmd = b.self_launch_cmd(["--gpus", "8", "--steps", "20", "--warmup", "5"], 8, 29417)
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert cmd[3:10] == ["--nnodes=1", "--nproc-per-node", "8", "--master-addr", "127.0.0.1", "--master-port", "29417"]
    assert os.path.basename(cmd[10]) == "bench.py" and os.path.isabs(cmd[10])
    assert cmd[11:] == ["--gpus", "8", "--steps", "20", "--warmup", "5"]
    # fewer GPUs than ranks: refused before anything is started
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit, match="shows 0 GPU"):
        b.self_launch(["--gpus", "2"], 2)
    # the job's stdout is passed through line by line, exit code returned
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 2)
    seen = {}

    class FakeProc:
        stdout = io.StringIO("banner\n{\"value\": 1}\n")

        def wait(self):
            return 0

    def popen(cmd_, env=None, **kw):
        seen["cmd"], seen["env"] = cmd_, env
        return FakeProc()
    monkeypatch.setattr(subprocess, "Popen", popen)
    out = io.StringIO()
    monkeypatch.setattr(sys, "stdout", out)
    assert b.self_launch(["--gpus", "2"], 2) == 0
    monkeypatch.undo()
    assert out.getvalue().splitlines()[-1] == '{"value": 1}'
    assert seen["cmd"][5] == "2" and seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def test_bench_dump_outputs_writes_the_step_results_as_float32(tmp_path):
    """--dump-outputs: the loss, the parameter and gradient arenas (FactorVAE: also the discriminator's) as <name>.npy, float32,
    within the 64 MB bound"""
    from disvae_amd.models.vae import init_specific_model
    from disvae_amd.models.discriminator import Discriminator
    b = _bench_module()
    model = init_specific_model("Burgess", (3, 64, 64), 10)
    model.arena.grad.normal_()

    class FactorLoss:
        discriminator = Discriminator(latent_dim=10)
    b.dump_outputs(str(tmp_path / "vae"), torch.tensor(3.5), model, object())
    b.dump_outputs(str(tmp_path / "factor"), torch.tensor(3.5), model, FactorLoss())
    assert sorted(os.listdir(tmp_path / "vae")) == ["grads.npy", "loss.npy", "params.npy"]
    names = sorted(os.listdir(tmp_path / "factor"))
    assert names == ["disc_grads.npy", "disc_params.npy", "grads.npy", "loss.npy", "params.npy"]
    arrays = {n: np.load(str(tmp_path / "factor" / n)) for n in names}
    assert all(a.dtype == np.float32 for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= b.MAX_DUMP_BYTES
    assert arrays["loss.npy"].tolist() == [3.5]
    assert np.array_equal(arrays["params.npy"], model.arena.flat.numpy())
    assert np.array_equal(arrays["grads.npy"], model.arena.grad.numpy())
    assert np.array_equal(arrays["disc_params.npy"], FactorLoss.discriminator.arena.flat.numpy())


def test_bench_cpu_baseline_leg_runs_the_port_and_calibrates_threads_once(monkeypatch):
    """the CPU leg (tier rule 4: a bounded sample of the same workload on the host cores) on a tiny batch; the thread count is
    probed once per process, never with more than 64 threads"""
    b = _bench_module()
    seen = []
    real, before = torch.set_num_threads, torch.get_num_threads()
    monkeypatch.setattr(torch, "set_num_threads", lambda n: (seen.append(n), real(min(n, 4)))[1])
    monkeypatch.setattr(b, "have_reference", lambda: False)
    cfg = dict(b.CONFIGS["btcvae_dsprites"])
    try:
        r1 = b.cpu_baseline(cfg, 8, iters=1, warm=0)
        n_probe = len(seen)
        r2 = b.cpu_baseline(cfg, 8, iters=1, warm=0)
    finally:
        real(before)
    assert r1["kind"] == "port" and r1["unit"] == "images/s" and r1["value"] > 0 and r1["cores"] == r2["cores"]
    assert max(seen) <= 64 or max(seen) <= (os.cpu_count() or 1)
    assert len(seen) - n_probe == 1, "the second leg re-uses the calibrated thread count"


def test_wide_latent_kernel_math_emulation():
    """tools/emu/latent_wide_math.py: the arithmetic and buffer layouts of csrc/latent_wide.hip (latent dimensions above 16)
    restated kernel by kernel in fp64 and held to the oracle -- whole batch, row shards, the wide packed / scalar layouts."""
    import runpy
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ns = runpy.run_path(os.path.join(root, "tools", "emu", "latent_wide_math.py"), run_name="__main__")
    assert ns["N_CASES"] == 3
    # the kernels read the layouts the emulation uses (include/dvae_hip.h macros, evaluated in tests/test_cabi_symbols.py)
    src = open(os.path.join(root, "disentangling-vae_amd", "csrc", "latent_wide.hip")).read()
    assert "DVAE_ROWSTATS_STRIDE(D)" in src and "tmp + (size_t)3 * D * Bg" in src


@pytest.mark.parametrize("script", ["thin_ws_index_math.py", "gemm_dma_index_math.py"])
def test_kernel_addressing_emulations(script):
    """tools/emu/*: lane-level numpy emulations of the LDS-DMA kernels' addressing (workgroup -> tile maps, per-lane transfer
    sources and masks, operand reads, MFMA lane layouts, epilogue / partial-buffer slots) against numpy references -- run
    here so that they stay runnable, and (thin kernels) with the layout constants checked against the source."""
    import re
    import runpy
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ns = runpy.run_path(os.path.join(root, "tools", "emu", script), run_name="__main__")
    if script.startswith("thin_ws"):
        # the emulation's layout constants are the kernels' (csrc/conv_thin_ws.hip: ThinWsGeo / ThinWgGeo)
        src = open(os.path.join(root, "disentangling-vae_amd", "csrc", "conv_thin_ws.hip")).read()
        planes = [int(v) for v in re.findall(r"static constexpr int PLANE = (\d+);", src)]
        zz = [int(v) for v in re.findall(r"static constexpr int ZZ = (\d+);", src)]
        assert planes == [ns["PLANE_D"], ns["PLANE_W"]] and zz == [ns["ZZ"], ns["ZZ"]], (planes, zz)


@pytest.mark.parametrize("loss", ["VAE", "betaH", "betaB", "factor", "btcvae"])
def test_any_latent_dim_is_accepted_for_every_loss(loss):
    """main.py:81 takes any --latent-dim and disvae/models/losses.py:523-544 is dimension-agnostic.  The fused HIP kernels
    cover 1..16 (include/dvae_hip.h: DVAE_MAX_D); above that the engine switches to the run-time-D kernels (csrc/latent_wide.hip,
    tests/test_gpu_wide_latent.py) -- nothing is refused and nothing is truncated: the model carries 2D / D-wide layers, the
    loss plugin's buffers follow the "wide" layouts.  What IS refused: values that are not positive integers."""
    from disvae_amd.models.vae import init_specific_model, VAE
    from disvae_amd.models.losses import get_loss_f
    from disvae_amd import _lib
    assert _lib.MAX_LATENT_DIM == 16
    for D in (0, -1, 2.5, "10", True, None):
        with pytest.raises(ValueError, match="latent_dim"):
            init_specific_model("Burgess", (1, 32, 32), D)
        with pytest.raises(ValueError, match="latent_dim"):
            VAE((3, 64, 64), latent_dim=D)
    for D in (1, 16, 17, 32, 100):
        m = init_specific_model("Burgess", (1, 32, 32), D)
        sd = m.state_dict()
        assert sd["encoder.mu_logvar_gen.weight"].shape == (2 * D, 256) and sd["decoder.lin1.weight"].shape == (256, D)
        assert (_lib.wide(D), _lib.kl0(D)) == ((False, _lib.S_KL0) if D <= 16 else (True, _lib.WIDE_KL0))
    hp = dict(rec_dist="bernoulli", reg_anneal=0, betaH_B=4, betaB_initC=0, betaB_finC=25, betaB_G=1000, factor_G=6.4,
              latent_dim=17, lr_disc=1e-4, btcvae_A=1, btcvae_B=6, btcvae_G=1, n_data=1000, device=torch.device("cpu"))
    loss_f = get_loss_f(loss, **hp)                                      # the plugin itself holds no latent-sized state
    if loss == "factor":
        assert loss_f.discriminator.state_dict()["lin1.weight"].shape == (1000, 17)
    # the logged scalars of a wide step: kl_loss_i is read at scal[DVAE_WIDE_KL0 + i]
    from collections import defaultdict
    st = defaultdict(list)
    vals = list(range(_lib.nscal(20)))
    type(loss_f)._store_kl(st, vals, 20)
    assert st["kl_loss_0"] == [32] and st["kl_loss_19"] == [51] and st["kl_loss"] == [_lib.S_KL]
    st = defaultdict(list)
    type(loss_f)._store_kl(st, vals, 10)
    assert st["kl_loss_0"] == [_lib.S_KL0] and st["kl_loss_9"] == [_lib.S_KL0 + 9]


def test_round6_schedule_policies():
    """Host-side decisions of round 6, no kernels: which steps carry the 8x8 <-> 4x4 conv layers inside the FC-chain launches
    (StepPolicy.fuse_ends, up to fuse_ends_max_rows rows; never above 16 latents, where there is no chain launch), which steps put
    their weight gradients on two side streams (FactorVAE from 2048 rows, the other losses never) and where convT3's weight
    gradient is forked; the dvae_fc_chain_*_args structs carry the conv-end fields behind the version-108 ones."""
    from disvae_amd import _lib, schedule as P
    from disvae_amd.engine import VAEEngine

    def policy(img, D, rows=128, **kw):
        return P.build_policy(img, D, rows, P.switches(), **kw)
    pol = policy((3, 64, 64), 10)
    assert pol.fuse_ends and pol.fuse_ends_max_rows == 256 and pol.fuse_ends_max_rows_fwd == 1024
    assert pol.early_thin_wgrad == 1 and pol.early_thin_auto and not pol.sharded and not pol.three_streams
    assert pol.ends(1) and pol.ends(256) and not pol.ends(257) and not pol.ends(1024)
    assert pol.ends_fwd(257) and pol.ends_fwd(1024) and not pol.ends_fwd(1025)
    assert policy((1, 32, 32), 10).fuse_ends          # conv3 / convT1 are that geometry's 4x4 end
    assert not policy((3, 64, 64), 17).fuse_ends      # per-layer FC launches above 16 latents
    # (model.engine refuses on a CPU model: the engine object itself is host-side state only)
    m = init_specific_model("Burgess", (3, 64, 64), 10)
    eng = VAEEngine(m.img_size, m.latent_dim, m.arena)
    eng.begin_step(pol._replace(three_streams=True))
    assert eng._three(True) and not eng._three(False)
    eng.begin_step(eng.policy._replace(single_stream=True))
    assert not eng._three(True)
    assert P.THREE_STREAM_MIN_ROWS > 1 << 20 and P.THREE_STREAM_MIN_ROWS_FACTOR == 2048
    for kind, rows, three in ((_lib.LOSS_FACTOR, 2048, True), (_lib.LOSS_FACTOR, 2046, False), (_lib.LOSS_BTCVAE, 2048, False),
                              (_lib.LOSS_BETAH, 4096, False)):
        assert policy((3, 64, 64), 10, rows, kind=kind).three_streams == three, (kind, rows)
    assert not policy((3, 64, 64), 10, 2048, kind=_lib.LOSS_FACTOR, world=2).three_streams      # single process only
    # where convT3's weight gradient is forked: mode 1, mode 2 at 112-128 rows of a single process, nowhere on one stream
    assert [pol.early_thin(r) for r in (111, 112, 128, 129)] == [1, 2, 2, 1]
    assert policy((3, 64, 64), 10, world=2).early_thin(128) == 1 and pol._replace(single_stream=True).early_thin(128) == 0
    assert [pol.fcw_main_at(r) for r in (128, 129, 320, 321)] == [False, True, True, False]
    # a policy is a value: equal inputs give the same object, and it is the replay key's entry for every decision
    assert policy((3, 64, 64), 10) is pol and hash(pol) == hash(pol._replace()) and pol != pol._replace(late_join=True)
    f = [n for n, _ in _lib.FcChainFwdArgs._fields_]
    b = [n for n, _ in _lib.FcChainBwdArgs._fields_]
    assert f[-6:] == ["conv_in", "conv_w", "conv_b", "convT_w", "convT_b", "convT_out"] and f[-7] == "D"
    assert b[-6:] == ["convT_gout", "convT_w", "d3", "conv_w", "conv_act", "conv_gin"] and b[-7] == "D"
