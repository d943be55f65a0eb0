"""-m gpu: the k-NN mutual-information library (lib_scores/libdvae_knn_hip.so, csrc/knn_mi.hip;
Evaluator.compute_knn_information_scores) against the numpy restatement of tests/knn_ref.py, which tests/test_knn_host.py holds to
scikit-learn's _compute_mi_cd bit for bit.

INTEGERS.  m_i, k_i (dumped by selection index), the class counts and n must equal the restatement's integer for integer: the
device works on sorted lists with exact fp64 differences, so there is nothing to tolerate.  Sizes (SIZE_CASES): S = 2, 63 / 64 / 65
(a wave), 255 / 256 / 257, 1000; 511 / 512 / 513 on both sides of the estimator's tile of 512 threads and of a power of two of the
sort's padding; 1023 / 1024 / 1025 on both sides of the sort's 1024 threads; DVAE_KNN_MAX_ROWS itself once.  The launcher has no
other switch.  Factors of 2, 3, 40 and 256 values; n_neighbors 1, 3 and 7.  Tables built to break a sort-and-search
(BREAK_CASES), each with K >= 2 and D >= 3 so that a mix-up of the workgroup indices shows: a constant column, a 2^-3 grid (equal
distances left and right: the strict `<`), +-0, denormals, 30 + 1e-3 noise, values that differ in the lowest mantissa bits,
repeated rows, a factor with some singleton labels and one with nothing else (n = 0), rows descending, shuffled and NULL.

SUMS.  The device and the restatement read the SAME psi table and add the same terms: only the order differs, so each of the three
sums must agree within 4 B, B = S 2^-53 sum |psi terms of that sum| (the project's first-order bound of a sum of S terms, times
the usual margin of 4).  The RAW estimate psi(n) + (sum_k - sum_c - sum_m) / n is compared too -- a pair that clips to 0 still
tests something -- within 4 (B_k + B_c + B_m) / n plus the rounding of its own seven operations on either side, 14 * 2^-53 *
(|psi(n)| + the three |means|).  Every ratio is printed; the worst is in DESIGN.md."""
import functools
import json
import logging
import os

import numpy as np
import pytest
import torch

import knn_ref as R
from gpu_util import DEV, stream
from guard_util import Guarded, run_contract
from disvae_amd import _knnlib, Evaluator, digamma_integers, knn_information_scores_from_mi, knn_information_scores_from_table

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
WIDE = (2, 3, 40, 256)                                                  # 61 440 rows
# (name, family, lat_sizes, D, S, rows: "shuffled" / "descending" / "repeats" / "all" (NULL) / "unique-last", n_neighbors, seed)
SIZE_CASES = [("S-%d" % S, "clusters", WIDE, 3, S, "shuffled", (1, 3, 7)[i % 3], 10 + i)
              for i, S in enumerate((2, 63, 64, 65, 255, 256, 257, 1000, 511, 512, 513, 1023, 1024, 1025))]
SIZE_CASES.append(("S-max-rows", "grid", WIDE, 3, _knnlib.MAX_ROWS, "shuffled", 3, 30))
BREAK_CASES = [
    ("constant-column", "constant", (3, 5, 40), 4, 600, "all", 3, 41),
    ("grid-2^-3", "grid", (3, 5, 40), 4, 600, "shuffled", 1, 42),
    ("grid-2^-3-k7", "grid", (3, 5, 40), 4, 577, "descending", 7, 43),
    ("signed-zeros", "zeros", (3, 5, 40), 4, 600, "shuffled", 3, 44),
    ("denormals", "denormal", (3, 5, 40), 4, 600, "shuffled", 3, 45),
    ("offset-30", "offset", (3, 5, 40), 4, 600, "descending", 3, 46),
    ("lowest-bits", "ulp", (3, 5, 40), 4, 600, "shuffled", 7, 47),
    ("repeated-rows", "clusters", (3, 5, 40), 4, 700, "repeats", 3, 48),
    ("some-singletons", "clusters", (3, 200), 3, 250, "shuffled", 3, 49),
    ("all-singletons", "noise", (3, 200), 3, 200, "unique-last", 3, 50),
]
CASES = SIZE_CASES + BREAK_CASES
IDS = [c[0] for c in CASES]


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype).contiguous()


@functools.lru_cache(maxsize=None)
def case(name):
    """The inputs of a case and the restatement's outputs, computed once."""
    _n, family, sizes, D, S, mode, kn, seed = CASES[IDS.index(name)]
    tab = R.table(family, sizes, D, seed=seed)
    N = tab.shape[0]
    rng = np.random.default_rng(seed)
    if mode == "shuffled":
        rows = rng.permutation(N)[:S]
    elif mode == "descending":
        rows = np.sort(rng.permutation(N)[:S])[::-1]
    elif mode == "repeats":
        rows = rng.integers(0, N // 2, S)
    elif mode == "all":
        rows = None
    else:                                                               # every value of the last factor once
        rows = np.arange(sizes[-1]) + sizes[-1] * (np.arange(sizes[-1]) % sizes[0])
    assert S == (N if rows is None else len(rows)) <= _knnlib.MAX_ROWS
    rows = None if rows is None else np.ascontiguousarray(rows, dtype=np.int64)
    psi = digamma_integers(S)
    ref = R.reference(tab, sizes, np.arange(N) if rows is None else rows, kn, psi)
    return dict(tab=tab, N=N, D=D, K=len(sizes), S=S, sizes=list(sizes), rows=rows, kn=kn, psi=psi, ref=ref)


def run(c, with_dumps=True, fill=float("nan")):
    """dvae_knn_sort + dvae_knn_mi on poisoned outputs -> (sums [D, K, 4], counts [K, sum sizes], m_of, k_of, ws as int32)."""
    D, K, S, sum_sizes = c["D"], c["K"], c["S"], sum(c["sizes"])
    td, pd = _dev(c["tab"], torch.float32), _dev(c["psi"], torch.float64)
    rd = None if c["rows"] is None else _dev(c["rows"], torch.int64)
    h = _knnlib.lib()
    assert h.dvae_knn_ws_bytes(c["N"], D, S if rd is not None else 0) == 8 * D * S
    ws = torch.full((2 * D * S,), -7, dtype=torch.int32, device=DEV)
    sums = torch.full((D, K, 4), fill, dtype=torch.float64, device=DEV)
    counts = torch.full((K, sum_sizes), -7, dtype=torch.int32, device=DEV)
    m_of = torch.full((D, K, S), -7, dtype=torch.int32, device=DEV) if with_dumps else None
    k_of = torch.full((D, K, S), -7, dtype=torch.int32, device=DEV) if with_dumps else None
    ptr = (lambda t: None if t is None else t.data_ptr())
    torch.cuda.synchronize()
    _knnlib.call("dvae_knn_sort", td.data_ptr(), ptr(rd), c["N"], D, S, ws.data_ptr(), stream())
    _knnlib.call("dvae_knn_mi", ptr(rd), _knnlib.host_sizes(c["sizes"]), c["N"], D, K, S, c["kn"], pd.data_ptr(), ws.data_ptr(),
                 sums.data_ptr(), counts.data_ptr(), ptr(m_of), ptr(k_of), stream())
    torch.cuda.synchronize()
    return (sums.cpu().numpy(), counts.cpu().numpy(), None if m_of is None else m_of.cpu().numpy(),
            None if k_of is None else k_of.cpu().numpy(), ws.cpu().numpy())


@functools.lru_cache(maxsize=None)
def device(name):
    return run(case(name))


def block_counts(counts, sizes):
    """[K, sum sizes] -> the K blocks; everything outside them must be 0."""
    out, start, rest = [], 0, counts.copy()
    for k, size in enumerate(sizes):
        out.append(counts[k, start:start + size])
        rest[k, start:start + size] = 0
        start += size
    assert not rest.any()
    return out


# ---- 1. integers and sums against the restatement ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", IDS)
def test_integers_equal_the_restatement(name):
    c = case(name)
    ref = c["ref"]
    sums, counts, m_of, k_of, ws = device(name)
    D, S = c["D"], c["S"]
    # the sort: the values ascending, the indices a permutation, and together the gathered column (-0 written as +0)
    sel = np.arange(c["N"]) if c["rows"] is None else c["rows"]
    vals, idx = ws[:D * S].view(np.float32).reshape(D, S), ws[D * S:].reshape(D, S)
    for d in range(D):
        assert (np.diff(vals[d].astype(np.float64)) >= 0).all() and np.array_equal(np.sort(idx[d]), np.arange(S))
        assert np.array_equal(vals[d], c["tab"][sel[idx[d]], d] + np.float32(0.0))
    for k, blk in enumerate(block_counts(counts, c["sizes"])):
        assert np.array_equal(blk, ref["counts"][k]), k
    assert np.array_equal(sums[:, :, 0], ref["n"].astype(np.float64))
    assert np.array_equal(k_of, ref["k_i"]) and np.array_equal(m_of, ref["m_i"])
    if name == "constant-column":
        assert (m_of[0] == ref["n"][0][:, None]).all() and (ref["n"][0] == S).all()       # every m_i = n
    if name == "all-singletons":
        assert (ref["n"][:, 1] == 0).all() and (sums[:, 1] == 0).all() and (ref["n"][:, 0] > 0).all()
    if name == "some-singletons":
        assert (0 < ref["n"][:, 1]).all() and (ref["n"][:, 1] < S).all()
    if name == "S-2":
        assert set(ref["n"].reshape(-1).tolist()) <= {0, 2}


@pytest.mark.parametrize("name", IDS)
def test_sums_and_raw_estimate_within_the_bound(name):
    c = case(name)
    ref = c["ref"]
    sums = device(name)[0]
    S, psi = c["S"], c["psi"]
    B = S * U * ref["bound"]                                             # [D, K, 3]
    err = np.abs(sums[:, :, 1:] - ref["sums"])
    ratio = float(np.max(err / np.maximum(B, 1e-300)))
    raw = R.raw_from_sums(np.rint(sums[:, :, 0]).astype(np.int64), sums[:, :, 1:], psi)
    n = np.maximum(ref["n"], 1)
    tol_raw = 4.0 * B.sum(axis=2) / n + 14.0 * U * (np.abs(psi[n]) + (np.abs(ref["sums"]) / n[:, :, None]).sum(axis=2))
    ratio_raw = float(np.max(np.abs(raw - ref["raw"]) / np.maximum(tol_raw, 1e-300)))
    clipped = int((ref["raw"] <= 0).sum())
    print("%s: S = %d, sums at most %.4f B (pass at 4), raw estimate at most %.4f of its tolerance, %d of %d pairs clip to 0, raw in [%.3f, %.3f]"
          % (name, S, ratio, ratio_raw, clipped, ref["raw"].size, ref["raw"].min(), ref["raw"].max()))
    assert np.isfinite(sums).all()
    assert (err <= 4.0 * B).all(), (name, ratio)
    assert (np.abs(raw - ref["raw"]) <= tol_raw).all(), (name, ratio_raw)


# ---- 2. determinism, memory -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["S-2", "S-513", "S-1025", "S-max-rows", "signed-zeros", "repeated-rows", "all-singletons"])
def test_same_bits_twice_and_without_the_dumps(name):
    c = case(name)
    a = device(name)
    b = run(c, fill=-1e300)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    sums, counts, m_of, k_of, _ws = run(c, with_dumps=False)
    assert m_of is None and k_of is None and sums.tobytes() == a[0].tobytes() and counts.tobytes() == a[1].tobytes()


def _call(name):
    return lambda args: _knnlib.call(name, *[a.ptr if isinstance(a, Guarded) else a for a in args])


@pytest.mark.parametrize("name", ["S-2", "S-65", "S-513", "S-1025", "constant-column", "some-singletons", "all-singletons"])
def test_memory_contract(name):
    """Guards untouched, inputs unchanged, every output element written, bits equal to the run on plain tensors whatever the
    surroundings hold (NaN at 256-byte alignment; -1e30 at the weakest alignment promised: the element's own)."""
    c = case(name)
    D, K, S, sum_sizes = c["D"], c["K"], c["S"], sum(c["sizes"])
    sizes = _knnlib.host_sizes(c["sizes"])
    rows = None if c["rows"] is None else torch.from_numpy(c["rows"])
    sums, counts, m_of, k_of, ws = device(name)

    def build_sort(al):
        return [al.inp("table", c["tab"], align=4), None if rows is None else al.inp("rows", rows, align=8), c["N"], D, S,
                al.out("ws", (2 * D * S,), dtype=torch.int32, align=4), stream()]
    runs = run_contract("dvae_knn_sort", build_sort, fn=_call("dvae_knn_sort"))
    assert runs[0].args[-1].t.cpu().numpy().tobytes() == ws.tobytes()

    def build_mi(al):
        return [None if rows is None else al.inp("rows", rows, align=8), sizes, c["N"], D, K, S, c["kn"],
                al.inp("psi", torch.from_numpy(c["psi"]), align=8, dtype=torch.float64), al.inp("ws", torch.from_numpy(ws), align=4),
                al.out("sums", (D, K, 4), dtype=torch.float64, align=8), al.out("class_counts", (K, sum_sizes), dtype=torch.int32, align=4),
                al.out("m_of", (D, K, S), dtype=torch.int32, align=4), al.out("k_of", (D, K, S), dtype=torch.int32, align=4), stream()]
    runs = run_contract("dvae_knn_mi", build_mi, fn=_call("dvae_knn_mi"))
    got = {g.name: g.t.cpu().numpy() for g in runs[0].args}
    assert got["sums"].tobytes() == sums.tobytes() and np.array_equal(got["class_counts"], counts)
    assert np.array_equal(got["m_of"], m_of) and np.array_equal(got["k_of"], k_of)


# ---- 3. end to end ------------------------------------------------------------------------------------------------------------------
GRID = (3, 4, 5, 6)


def _end_to_end_table(name):
    ideal = R.table("clusters", GRID, 4, seed=3)                          # latent d follows factor d
    if name == "rotated":
        c = np.float32(np.sqrt(0.5))
        ideal[:, 0], ideal[:, 1] = c * (ideal[:, 0] - ideal[:, 1]), c * (ideal[:, 0] + ideal[:, 1])
    if name == "collapsed":
        ideal[:, 2:] = 0.5
    return ideal


def _assert_matches_restatement(got, tab, rows, kn):
    psi = digamma_integers(len(rows))
    ref = R.reference(tab, GRID, rows, kn, psi)
    assert np.array_equal(got["n_kept"], ref["n"]) and got["n_samples"] == len(rows) and got["n_neighbors"] == kn
    H = np.array([R.factor_entropy(cnt) for cnt in ref["counts"]])
    assert np.allclose(got["factor_entropy"], H, rtol=0, atol=1e-14)
    n = np.maximum(ref["n"], 1)
    tol = 4.0 * len(rows) * U * ref["bound"].sum(axis=2) / n + 14.0 * U * (np.abs(psi[n]) + (np.abs(ref["sums"]) / n[:, :, None]).sum(axis=2))
    assert (np.abs(got["raw"] - ref["raw"]) <= tol).all()
    assert np.array_equal(got["mutual_information"], np.maximum(got["raw"], 0.0))
    want = R.scores(got["raw"], got["factor_entropy"])                     # the restatement's formulas on the device's own sums
    for key in ("mig", "mig_sup", "dcimig", "modularity", "infom", "infoc"):
        assert abs(got[key] - want[key]) <= 1e-12, (key, got[key], want[key])
    assert got["n_active"] == want["n_active"] and np.array_equal(got["best_latent"], want["best_latent"])
    again = knn_information_scores_from_mi(got["raw"], got["factor_entropy"])
    assert all(again[key] == got[key] for key in ("mig", "infom", "infoc"))


def test_from_table_on_ideal_rotated_and_collapsed_tables():
    rows = np.random.default_rng(5).permutation(360)[:300]
    scores = {}
    cpu0, dev0 = torch.get_rng_state(), torch.cuda.get_rng_state()
    for name in ("ideal", "rotated", "collapsed"):
        tab = _end_to_end_table(name)
        got = knn_information_scores_from_table(_dev(tab, torch.float32), GRID, rows=rows)
        _assert_matches_restatement(got, tab, rows, 3)
        assert got["raw"].shape == got["mutual_information"].shape == got["n_kept"].shape == (4, 4) and isinstance(got["mig"], float)
        scores[name] = got
        print("%s: mig %.4f infom %.4f infoc %.4f modularity %.4f, %d active" % (name, got["mig"], got["infom"], got["infoc"],
                                                                                  got["modularity"], got["n_active"]))
    assert scores["ideal"]["best_latent"].tolist() == [0, 1, 2, 3]
    for key in ("mig", "infom"):
        assert scores["rotated"][key] < scores["ideal"][key]
    assert scores["collapsed"]["n_active"] <= 2 and (scores["collapsed"]["mutual_information"][2:] == 0).all()
    # the seeded selection: the same seed gives the same bits, the global random states are untouched
    td = _dev(_end_to_end_table("ideal"), torch.float32)
    a = knn_information_scores_from_table(td, GRID, n_samples=200, seed=3)
    b = knn_information_scores_from_table(td, GRID, n_samples=200, seed=3)
    other = knn_information_scores_from_table(td, GRID, n_samples=200, seed=4)
    assert torch.equal(torch.get_rng_state(), cpu0) and torch.equal(torch.cuda.get_rng_state(), dev0)
    assert a["raw"].tobytes() == b["raw"].tobytes() and a["raw"].tobytes() != other["raw"].tobytes()
    drawn = torch.randperm(360, generator=torch.Generator(device=DEV).manual_seed(3), device=DEV)[:200].cpu().numpy()
    _assert_matches_restatement(a, _end_to_end_table("ideal"), drawn, 3)
    every = knn_information_scores_from_table(td, GRID, n_samples=None, n_neighbors=1)       # every row, rows = NULL
    _assert_matches_restatement(every, _end_to_end_table("ideal"), np.arange(360), 1)
    twice = knn_information_scores_from_table(td, GRID, rows=np.concatenate([rows, rows]))  # a repeated row is another row
    _assert_matches_restatement(twice, _end_to_end_table("ideal"), np.concatenate([rows, rows]), 3)
    with pytest.raises(ValueError, match=r"factor\(s\) \[0\] take one value among the selected rows"):
        knn_information_scores_from_table(td, GRID, rows=np.arange(100))      # rows 0 .. 99: factor 0 is 0 throughout
    with pytest.raises(ValueError, match="NaN or an infinity"):
        bad = td.clone()
        bad[7, 2] = float("inf")
        knn_information_scores_from_table(bad, GRID, n_samples=100)
    with pytest.raises(ValueError, match=r"rows must hold between 1 and %d" % _knnlib.MAX_ROWS):
        knn_information_scores_from_table(td, GRID, rows=np.zeros(_knnlib.MAX_ROWS + 1, dtype=np.int64))


class _TableModel(torch.nn.Module):
    """A model whose encoder looks q(z|x) up in a table: image x is its row number."""

    def __init__(self, mean):
        super().__init__()
        self.latent_dim = mean.shape[1]
        self.register_buffer("mean", torch.from_numpy(np.ascontiguousarray(mean)))
        self.modes = []

    def encoder(self, x):
        self.modes.append(self.training)
        idx = x.view(-1).long()
        return self.mean[idx], torch.zeros_like(self.mean[idx])


class _Factors:
    lat_sizes, lat_names = np.array(GRID), tuple("abcd")

    def __len__(self):
        return 360


class _Loader:
    dataset = _Factors()

    def __iter__(self):
        for lo in range(0, 360, 100):
            yield torch.arange(lo, min(lo + 100, 360), dtype=torch.float32).view(-1, 1), None


def test_evaluator_end_to_end(tmp_path):
    tab = _end_to_end_table("ideal")
    model = _TableModel(tab).train()
    ev = Evaluator(model, None, device=torch.device(DEV), logger=logging.getLogger("knn"), save_dir=str(tmp_path), is_progress_bar=False)
    kw = dict(n_samples=300, n_neighbors=3, seed=2)
    got = ev.compute_knn_information_scores(_Loader(), **kw)
    again = ev.compute_knn_information_scores(_Loader(), **kw)
    assert model.training and model.modes == [False] * 8                     # encoded in eval mode, mode restored
    assert got["raw"].tobytes() == again["raw"].tobytes() and got["mig"] == again["mig"]
    direct = knn_information_scores_from_table(_dev(tab, torch.float32), GRID, **kw)
    assert direct["raw"].tobytes() == got["raw"].tobytes() and direct["infom"] == got["infom"] and direct["mig"] == got["mig"] > 0.3
    assert ev(_Loader(), is_losses=False) == (None, None) and os.listdir(tmp_path) == []
    assert ev(_Loader(), is_losses=False, is_knn_information=True, knn_information_args=kw) == (None, None)
    assert os.listdir(tmp_path) == ["knn_information_scores.log"]
    logged = json.load(open(tmp_path / "knn_information_scores.log"))
    assert set(logged) == set(got) - {"mutual_information", "raw", "n_kept"}
    assert logged["mig"] == got["mig"] and logged["infom"] == got["infom"] and logged["infoc"] == got["infoc"]
    assert logged["best_latent"] == got["best_latent"].tolist() and logged["n_samples"] == 300
    assert model.training and not any(model.modes)
    with pytest.raises(ValueError, match=r"n_samples must be at most 360"):
        ev.compute_knn_information_scores(_Loader())                         # the default wants 10 000 rows

    class _NoFactors:
        dataset = [0, 1, 2, 3]
    with pytest.raises(ValueError, match="Dataset needs to have known true factors of variations to compute the metric"):
        ev.compute_knn_information_scores(_NoFactors())
