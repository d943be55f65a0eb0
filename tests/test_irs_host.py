"""CPU: the host side of the interventional robustness score -- the fifth library's C-ABI (include/dvae_irs_hip.h ==
disvae_amd/_irslib.py == the built libdvae_irs_hip.so), the build, the value -> group map against numpy.digitize /
numpy.histogram, the fp64 restatement (tests/irs_ref.py) on tables whose score is known, the host combination of evaluate.py
against the restatement, the precondition of the GPU tests' end-to-end bound, and the argument errors raised before any library
call."""
import ctypes
import importlib
import importlib.util
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import info_ref as I
import irs_ref as R
from disvae_amd import _evallib, _infolib, _irslib, _lib, _scorelib, Evaluator
from disvae_amd.evaluate import irs_from_statistics, irs_from_table, irs_group_map, irs_quantile_ranks
from disvae_amd.models.losses import get_loss_f
from disvae_amd.models.vae import init_specific_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dvae_irs_hip.h")
KERNELS = ("k_irs_means_part", "k_irs_means_finish", "k_irs_select_init", "k_irs_select_hist", "k_irs_select_walk",
           "k_irs_select_next", "k_irs_select_finish")
HP = dict(rec_dist="bernoulli", reg_anneal=0, betaH_B=4, betaB_initC=0, betaB_finC=25, betaB_G=1000, factor_G=6.4,
          latent_dim=4, lr_disc=1e-4, btcvae_A=1, btcvae_B=6.4, btcvae_G=1)


# ---- 1. the library -----------------------------------------------------------------------------------------------------------
def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _nm(path, *flags):
    nm = shutil.which("nm") or shutil.which("llvm-nm", path="/opt/rocm/llvm/bin")
    assert nm, "no nm on this machine"
    return subprocess.run([nm] + list(flags) + [path], capture_output=True, text=True, check=True).stdout


def test_header_ctypes_table_and_exports_agree():
    declared = sorted(set(re.findall(r"\b(dvae_irs_[a-zA-Z0-9_]+)\s*\(", _header())))
    assert declared == sorted(_irslib.SIGNATURES) and len(declared) == 6
    exported = sorted(set(re.findall(r" T (dvae_\w+)", _nm(os.path.abspath(_irslib.LIB_PATH), "-D", "--defined-only"))))
    assert exported == declared
    kinds = {ctypes.c_void_p: "p", ctypes.c_int: "i", ctypes.c_long: "l"}
    for name, params in re.findall(r"\b(dvae_irs_[a-zA-Z0-9_]+)\s*\(([^)]*)\)", _header()):
        got = []
        for prm in [x.strip() for x in params.split(",") if x.strip() != "void"]:
            got.append("p" if "*" in prm else ("l" if prm.startswith("long") else "i"))
        assert got == [kinds[t] for t in _irslib.SIGNATURES[name]], name
    macros = {k: int(v) for k, v in re.findall(r"#define (DVAE_IRS_\w+) (\d+)", _header())}
    mirrored = {"DVAE_IRS_VERSION": _irslib.VERSION, "DVAE_IRS_MAX_FACTORS": _irslib.MAX_FACTORS,
                "DVAE_IRS_MAX_GROUPS": _irslib.MAX_GROUPS, "DVAE_IRS_MEANS_COLS": _irslib.MEANS_COLS,
                "DVAE_IRS_MEANS_BLOCK_ROWS": _irslib.MEANS_BLOCK_ROWS, "DVAE_IRS_SELECT_BLOCK_ROWS": _irslib.SELECT_BLOCK_ROWS,
                "DVAE_IRS_MAX_BLOCKS": _irslib.MAX_BLOCKS, "DVAE_IRS_SELECT_LDS_GROUPS": _irslib.SELECT_LDS_GROUPS,
                "DVAE_IRS_SELECT_PASSES": _irslib.SELECT_PASSES, "DVAE_IRS_MAX_PAIRS": _irslib.MAX_PAIRS}
    assert macros == mirrored                                            # every macro of the header, none besides
    assert _irslib.MAX_FACTORS == 8 and _irslib.MAX_GROUPS >= 183        # dSprites' 40 and a 183-valued factor pass unbinned
    assert _irslib.SELECT_PASSES * 8 == 32                               # the passes cover the 32 bits of a deviation
    assert _irslib.lib().dvae_irs_version() == _irslib.VERSION == 1


def test_argument_errors_are_reported_before_any_launch():
    h = _irslib.lib()
    dummy = 1 << 20                                               # aligned non-NULL address, never dereferenced
    #           table  rows   sizes  map    groups N   D  K  S   sum tot max ws     counts means  stream
    means = [dummy, dummy, dummy, dummy, dummy, 60, 3, 3, 10, 12, 13, 5, dummy, dummy, dummy, None]
    #           table  rows   sizes  map    groups centre rank   N   D  K  S   sum tot max ws     lo     hi     mx     stream
    stats = [dummy, dummy, dummy, dummy, dummy, dummy, dummy, 60, 3, 3, 10, 12, 13, 5, dummy, dummy, dummy, dummy, None]
    bad = []
    # o: where N stands; then D, K, S, sum_sizes, total_groups, max_groups
    entries = (("dvae_irs_group_means", means, (0, 2, 3, 4, 12, 13, 14), 5), ("dvae_irs_group_order_stats", stats, (0, 2, 3, 4, 5, 6, 14, 15, 16, 17), 7))

    def put(good, i, v):
        return good[:i] + [v] + good[i + 1:]
    for name, good, ptrs, o in entries:
        for i in ptrs:
            bad.append((name, put(good, i, None)))
        for i in range(o, o + 7):
            bad += [(name, put(good, i, 0)), (name, put(good, i, -1))]
        bad.append((name, put(good, o + 2, _irslib.MAX_FACTORS + 1)))                 # the two limits
        bad.append((name, put(good, o + 6, _irslib.MAX_GROUPS + 1)))
        bad.append((name, put(good, o + 4, 2)))                                       # fewer values than factors
        bad.append((name, put(good, o + 5, 3)))                                       # fewer groups than 1 + K
        bad.append((name, put(good, o + 5, 17)))                                      # more than 1 + K max_groups
        bad.append((name, put(good, o + 1, _irslib.MAX_PAIRS // 13 + 1)))             # total_groups * D over the limit
    for name, args in bad:
        with pytest.raises(_lib.DvaeHipError, match="invalid argument"):
            _irslib.call(name, *args)
        assert b"invalid argument" in h.dvae_irs_last_error()
    for name, good, _ptrs, o in entries:
        with pytest.raises(_lib.DvaeHipError, match="DVAE_IRS_MAX_FACTORS"):
            _irslib.call(name, *put(good, o + 2, 9))
        with pytest.raises(_lib.DvaeHipError, match="DVAE_IRS_MAX_GROUPS"):
            _irslib.call(name, *put(good, o + 6, 257))


def test_workspace_sizes_are_what_the_header_promises():
    h = _irslib.lib()
    mws, sws = h.dvae_irs_group_means_ws_floats, h.dvae_irs_group_order_stats_ws_floats
    for N, D, K, S, G in ((0, 10, 5, 4, 20), (5, 0, 5, 4, 20), (5, 10, 0, 4, 20), (-1, 10, 5, 4, 20), (5, -3, 5, 4, 20), (5, 10, -7, 4, 20),
                          (5, 10, 9, 4, 20), (5, 10, 5, 4, 5), (5, 10, 5, 4, 0), (5, 10, 2, 4, 2 + 2 * _irslib.MAX_GROUPS),
                          (5, _irslib.MAX_PAIRS // 20 + 1, 5, 4, 20)):
        assert mws(N, D, K, S, G) == 0 and sws(N, D, K, S, G) == 0
    # means: one record of (2 D + 1) total_groups words per chunk; S <= 0: all N rows; the grid stops at MAX_BLOCKS chunks
    rec = (2 * 10 + 1) * 114
    assert mws(737280, 10, 5, 0, 114) == mws(737280, 10, 5, 737280, 114) == _irslib.MAX_BLOCKS * rec
    assert mws(60, 10, 5, 1, 114) == rec and mws(60, 10, 5, _irslib.MEANS_BLOCK_ROWS + 1, 114) == 2 * rec
    assert mws(60, 10, 5, 1 << 30, 114) == _irslib.MAX_BLOCKS * rec
    # selection: 256 counters and 5 words of state per (group, latent) pair, whatever S
    assert sws(737280, 10, 5, 0, 114) == sws(60, 10, 5, 7, 114) == 114 * 10 * (256 + 5)


# ---- 2. the build -------------------------------------------------------------------------------------------------------------
def test_build_leaves_five_libraries_and_keeps_them_apart():
    g = importlib.import_module("__graft_entry__")
    g.build()
    main, ev, sc, info, irs = (os.path.abspath(m.LIB_PATH) for m in (_lib, _evallib, _scorelib, _infolib, _irslib))
    assert os.path.dirname(main) == os.path.dirname(irs) and os.path.basename(irs) == "libdvae_irs_hip.so"
    assert all(os.path.exists(p) for p in (main, ev, sc, info, irs)) and len({main, ev, sc, info, irs}) == 5
    spec = importlib.util.spec_from_file_location("dvae_build_irs", os.path.join(ROOT, "disentangling-vae_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.IRS_SOURCES == ["factor_irs"]
    assert not set(mod.IRS_SOURCES) & set(mod.SOURCES + mod.EVAL_SOURCES + mod.SCORE_SOURCES + mod.INFO_SOURCES)
    assert os.path.abspath(mod.IRS_LIB) == irs and any(h.endswith("dvae_irs_hip.h") for h in mod.IRS_HEADERS)
    assert os.path.abspath(mod.build(verbose=False)) == main      # still the training library's path
    assert open(os.path.join(mod.OBJ, "flags_irs.txt")).read() == " ".join(mod.FLAGS + mod.IRS_SOURCES)
    others = [_nm(p, "-C") for p in (main, ev, sc, info)]
    in_irs = _nm(irs, "-C")
    for k in KERNELS:
        assert all(not re.search(r"\b%s\b" % k, text) for text in others), k
        assert re.search(r"__device_stub__%s\b" % k, in_irs), k + " is not in libdvae_irs_hip.so"
    assert all("dvae_irs_" not in text and "k_irs_" not in text for text in others)
    assert not any(s in in_irs for s in ("dvae_score_", "dvae_eval_", "dvae_info_", "k_info_"))


# ---- 3. the value -> group map --------------------------------------------------------------------------------------------------
def test_group_map_is_numpy_digitize_on_numpy_histogram():
    for bins in (1, 2, 20, 64):
        for size in range(1, 201):
            gmap, n_groups = irs_group_map([size], bins)
            label = np.digitize(np.arange(size), np.histogram(np.arange(size), bins)[1][:-1])
            uniq, dense = np.unique(label, return_inverse=True)
            assert gmap.dtype == np.int32 and np.array_equal(gmap, dense.reshape(-1)) and n_groups == [len(uniq)], (size, bins)
            assert n_groups[0] == min(size, bins) or size > bins                 # every value its own group while they fit
            assert (np.diff(gmap) >= 0).all() and gmap[0] == 0                   # monotone: a bin is a run of values
    gmap, n_groups = irs_group_map([3, 6, 40, 32, 32], None)
    assert n_groups == [3, 6, 40, 32, 32] and np.array_equal(gmap, np.concatenate([np.arange(s) for s in (3, 6, 40, 32, 32)]))
    gmap, n_groups = irs_group_map([3, 6, 40, 32, 32], 20)
    assert n_groups == [3, 6, 20, 20, 20] and len(gmap) == 113
    assert R.group_layout((3, 6, 40, 32, 32), 20)[1] == n_groups and np.array_equal(R.group_layout((3, 6, 40, 32, 32), 20)[0], gmap)


# ---- 4. the restatement -------------------------------------------------------------------------------------------------------
# the numpy restatement on the tables of tests/info_ref.py: 1.0 / 0.6923 / 0.2967 and 1.0 / 0.9066 / 0.3451 to four digits
KNOWN = {((3, 4, 5), 3): (1.0, 0.6923214859787573, 0.2966731433146633),
         ((2, 3, 6, 20), 7): (1.0, 0.9066295491793189, 0.34510379827252713)}


@pytest.mark.parametrize("lat_sizes,D", sorted(KNOWN))
def test_reference_irs_of_known_tables(lat_sizes, D):
    ideal, rotated, gauss = (R.irs(t, lat_sizes) for t in (I.ideal_table(lat_sizes, D), I.rotated_table(lat_sizes, D),
                                                            I.make_table(lat_sizes, D, "gauss")))
    assert ideal["IRS"] == 1.0 and (ideal["disentanglement_scores"] == 1.0).all()
    assert list(ideal["parents"]) == list(range(len(lat_sizes))) and ideal["active"].sum() == len(lat_sizes)
    assert rotated["IRS"] < 1.0 and gauss["IRS"] < rotated["IRS"]
    for got, want in zip((ideal, rotated, gauss), KNOWN[(lat_sizes, D)]):
        assert abs(got["IRS"] - want) <= 1e-12 and round(got["IRS"], 4) == round(want, 4)


def test_reference_constant_tables_and_inactive_columns():
    lat = (3, 4, 5)
    const = R.irs(I.make_table(lat, 4, "const"), lat)
    assert const["IRS"] == 0.0 and not const["active"].any() and const["IRS_matrix"].shape == (0, 3)
    table = I.make_table(lat, 3, "gauss")
    padded = np.concatenate([table[:, :1], np.full((60, 2), 0.3, dtype=np.float32), table[:, 1:], np.zeros((60, 1), dtype=np.float32)], axis=1)
    a, b = R.irs(table, lat), R.irs(padded, lat)
    assert a["IRS"] == b["IRS"] and np.array_equal(a["IRS_matrix"], b["IRS_matrix"])
    assert list(b["active"]) == [True, False, False, True, True, False]


def _fp64_statistics(table, lat, fb, q, rows):
    """the restatement's own statistics in the layout of dvae_irs_group_order_stats: fp64 centres, fp64 deviations, numpy.sort"""
    x, _ = I.select(table, lat, rows)
    x64 = x.astype(np.float64)
    masks, n_groups = R.group_masks(lat, fb, rows)
    counts = masks.sum(axis=1)
    rank, _t = irs_quantile_ranks(counts, q)
    lo, hi, mx = (np.zeros((len(counts), x.shape[1])) for _ in range(3))
    for g, m in enumerate(masks):
        if m.any():
            dev = np.sort(np.abs(x64[m] - x64[m].mean(axis=0)), axis=0)
            lo[g], hi[g], mx[g] = dev[rank[g]], dev[min(rank[g] + 1, len(dev) - 1)], dev[-1]
    return counts, n_groups, lo, hi, mx


def test_host_combination_is_the_restatement():
    one_row_group = np.array([0, 1, 2, 3, 20, 59])                 # factor 0 of (3, 4, 5): value 1 once, value 2 once
    leaves_a_group_empty = np.arange(0, 40)                        # ... value 2 never
    cases = [(k, lat, D, fb, q, R.rows_of(int(np.prod(lat)), D, S)) for k, lat, D, fb, q, S in R.END_TO_END]
    cases += [("gauss", (3, 4, 5), 3, 20, q, None) for q in (0.0, 1.0, 0.5, 0.37)]
    cases += [("gauss", (3, 4, 5), 3, 20, R.Q, one_row_group), ("rotated", (3, 4, 5), 4, None, 0.5, leaves_a_group_empty),
              ("gauss", (2, 3, 6, 20), 7, 4, 0.0, leaves_a_group_empty), ("gauss", (3, 4, 5), 3, 20, 1.0, np.array([7]))]
    for kind, lat, D, fb, q, rows in cases:
        table = R.end_to_end_table(kind, lat, D)
        ref = R.irs(table, lat, q, fb, rows)
        counts, n_groups, lo, hi, mx = _fp64_statistics(table, lat, fb, q, rows)
        if rows is leaves_a_group_empty:
            assert (counts == 0).any()
        if rows is one_row_group:
            assert (counts == 1).any()
        got = irs_from_statistics(counts, n_groups, lo, hi, mx, q)
        assert set(got) == set(ref)
        for key in ref:
            np.testing.assert_allclose(got[key], ref[key], rtol=0, atol=1e-12, err_msg="%s %s %s" % (kind, lat, key))
        assert np.array_equal(got["parents"], ref["parents"]) and np.array_equal(got["active"], ref["active"])
    single = irs_from_statistics(*_fp64_statistics(I.make_table((3, 4, 5), 3, "gauss"), (3, 4, 5), 20, 1.0, np.array([7])), 1.0)
    assert single["IRS"] == 0.0 and not single["active"].any()    # one selected row: every deviation is 0


def test_quantile_ranks_are_numpy_percentiles():
    rng = np.random.default_rng(2)
    for n in (1, 2, 3, 7, 100, 101, 18432):
        x = np.sort(rng.standard_normal(n))
        for q in (0.0, 0.01, 0.37, 0.5, 0.99, 1.0):
            lo, t = irs_quantile_ranks(np.array([n]), q)
            a, b = x[lo[0]], x[min(lo[0] + 1, n - 1)]
            mine = b - (b - a) * (1 - t[0]) if t[0] >= 0.5 else a + (b - a) * t[0]
            assert mine == np.percentile(x, 100 * q) and lo[0] == R.quantile_rank(n, q), (n, q)
    assert list(irs_quantile_ranks(np.array([0, 1, 5]), 0.99)[0]) == [-1, 0, 3]


# ---- 5. the precondition of the GPU tests' end-to-end bound --------------------------------------------------------------------
def test_fp32_path_stays_within_a_quarter_of_the_end_to_end_bound():
    """For every end-to-end case of tests/test_gpu_irs.py the restatement with fp32-rounded centres and fp32 deviations stays
    within a quarter of 4 * 2^-24 max|table| / max_deviations[d] of the pure fp64 one (worst 0.17: gauss on (3, 4, 5)), so the
    bound tests the kernels and not the definition."""
    worst = 0.0
    for kind, lat, D, fb, q, S in R.END_TO_END:
        table = R.end_to_end_table(kind, lat, D)
        rows = R.rows_of(table.shape[0], D, S)
        ref, low = R.irs(table, lat, q, fb, rows), R.irs(table, lat, q, fb, rows, fp32_path=True)
        if not ref["active"].any():
            assert low["IRS"] == 0.0
            continue
        ratio = R.worst_ratio(low, ref, R.matrix_bound(table, ref))
        worst = max(worst, ratio)
        assert ratio <= 0.25, (kind, lat, D, fb, q, S, ratio)
    print("worst fp32-path error / bound %.3f" % worst)


# ---- 6. errors before any library call ----------------------------------------------------------------------------------------
class _Factors:
    lat_sizes = np.array([3, 2])
    lat_names = ("a", "b")

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


class _Loader:
    def __init__(self, dataset, batches):
        self.dataset, self.batches = dataset, batches

    def __iter__(self):
        if self.batches is None:
            raise AssertionError("iterated before the sizes were checked")
        return iter(self.batches)


def test_argument_errors_raise_before_any_library_call(monkeypatch):
    def no_library():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_irslib, "lib", no_library)
    table = torch.zeros(6, 4)
    for args, kw, msg in ((([3, 3],), {}, "does not enumerate"), (([3, 2],), dict(diff_quantile=1.5), r"diff_quantile must lie in \[0, 1\]"),
                          (([3, 2],), dict(diff_quantile=-0.1), r"diff_quantile must lie in \[0, 1\]"),
                          (([3, 2],), dict(factor_bins=0), "factor_bins must be >= 1"), (([1] * 8 + [6],), {}, "at most 8"),
                          (([3, 2],), dict(n_samples=7), r"n_samples must lie in \[1, 6\]"),
                          (([3, 2],), dict(n_samples=0), r"n_samples must lie in \[1, 6\]"), (([3, 2],), dict(rows=[0, 6]), r"in \[0, 6\)"),
                          (([3, 2],), dict(rows=[-1]), r"in \[0, 6\)"), (([3, 2],), dict(rows=[]), "one row number or more"),
                          (([0, 2],), {}, "positive sizes")):
        with pytest.raises(ValueError, match=msg):
            irs_from_table(table, *args, **kw)
    with pytest.raises(ValueError, match="at most %d" % _irslib.MAX_GROUPS):
        irs_from_table(torch.zeros(257, 1), [257], factor_bins=None)
    with pytest.raises(ValueError, match="table"):
        irs_from_table(torch.zeros(6), [3, 2])
    bad = table.clone()
    bad[4, 1] = float("nan")
    with pytest.raises(ValueError, match="NaN"):
        irs_from_table(bad, [3, 2])
    with pytest.raises(_lib.DvaeHipError, match="no CPU"):
        irs_from_table(table, [3, 2])
    model = init_specific_model("Burgess", (1, 32, 32), 4)              # on the CPU: any device work would raise DvaeHipError
    ev = Evaluator(model, get_loss_f("VAE", **HP), device=torch.device("cpu"), is_progress_bar=False)
    with pytest.raises(ValueError, match="known true factors"):
        ev.compute_irs(_Loader([0, 1, 2], None))
    for kw, msg in ((dict(diff_quantile=2), "diff_quantile must lie"), (dict(n_samples=7), "n_samples must lie"),
                    (dict(factor_bins=-3), "factor_bins must be")):
        with pytest.raises(ValueError, match=msg):
            ev.compute_irs(_Loader(_Factors(6), None), **kw)
    with pytest.raises(ValueError, match=r"data set of 5 images does not enumerate lat_sizes=\[3, 2\]"):
        ev.compute_irs(_Loader(_Factors(5), None))
    model.train()
    loader = _Loader(_Factors(6), [(torch.rand(4, 1, 32, 32), None), (torch.rand(2, 1, 32, 32), None)])
    with pytest.raises(_lib.DvaeHipError):                              # valid arguments: the native encoder refuses the CPU
        ev.compute_irs(loader)
    assert model.training                                               # ... and the mode is as it was
