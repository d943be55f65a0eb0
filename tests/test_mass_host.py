"""CPU: the host side of the RMIG / JEMMIG / MIG-sup / DCIMIG interpretability scores -- the twelfth library's C-ABI
(include/dvae_mass_hip.h == disvae_amd/_masslib.py == the built lib/ext/libdvae_mass_hip.so), its row of build.py's EXTRA_TARGETS
(the other three lists, the 31 sources and the eleven libraries of lib/ untouched), the rules its source obeys, the refusal of bad
arguments before any launch, the workspace size, the restatement tests/mass_ref.py against scipy and mpmath (which pins U_REF),
the tail-difference rule, evaluate.interpretability_scores_from_mass on hand-made tables, the thresholds of the end-to-end GPU
test on the reference alone, and the argument errors of the public functions before any device work.

Measured here:
    math.erfc against mpmath (40 digits) over the erfc arguments of the GPU test's tables: at most 2.996 ulp  (U_REF = 3)
    far / sharp table (720 + 720 rows, 100 bins): Phi(b) - Phi(a) relative error up to 2.5 on cells above 1e-30 (3869 cells at
    0.5 or more); the tail form's row sums within 2 * 2^-53 of 1
    ideal table   mean rmig_norm 1.000, mean jemmig_norm 0.931;   rotated table   mean rmig_norm 0.125, mean jemmig_norm 0.122
"""
import ctypes
import importlib.util
import json
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import mass_ref as R
import disvae_amd
from disvae_amd import _cabi, _infolib, _lib, _masslib
from disvae_amd import evaluate as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dvae_mass_hip.h")
CSRC = os.path.join(ROOT, "disentangling-vae_amd", "csrc")
SOURCE = "posterior_mass.hip"
DUMMY = 1 << 20                                                   # aligned non-NULL address, never dereferenced
#        mean   logvar rows   sizes  edges  N  D  K  S  nb sum ws     mass   stream
JOINT = [DUMMY, DUMMY, DUMMY, DUMMY, DUMMY, 6, 3, 2, 4, 8, 5, DUMMY, DUMMY, None]
CASES = R.cases(_masslib.MAX_BINS, _masslib.BLOCK_ROWS, _masslib.MAX_CHUNKS, _masslib.LDS_DOUBLES)


def _build():
    spec = importlib.util.spec_from_file_location("dvae_build_mass", os.path.join(ROOT, "disentangling-vae_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _nm(path, *flags):
    nm = shutil.which("nm") or shutil.which("llvm-nm", path="/opt/rocm/llvm/bin")
    assert nm, "no nm on this machine"
    return subprocess.run([nm] + list(flags) + [path], capture_output=True, text=True, check=True).stdout


# ---- 1. the library -----------------------------------------------------------------------------------------------------------
def test_header_ctypes_table_and_exports_agree(monkeypatch):
    declared = sorted(set(re.findall(r"\b(dvae_mass_[a-zA-Z0-9_]+)\s*\(", _header())))
    assert declared == sorted(_masslib.SIGNATURES)
    assert declared == sorted(["dvae_mass_version", "dvae_mass_last_error", "dvae_mass_ws_doubles", "dvae_mass_joint"])
    exported = sorted(set(re.findall(r" T (dvae_\w+)", _nm(os.path.abspath(_masslib.LIB_PATH), "-D", "--defined-only"))))
    assert exported == declared
    assert re.findall(r" U (dvae_\w+)", _nm(os.path.abspath(_masslib.LIB_PATH), "-D")) == []
    kinds = {ctypes.c_void_p: "p", ctypes.c_int: "i", ctypes.c_long: "l"}
    for name, params in re.findall(r"\b(dvae_mass_[a-zA-Z0-9_]+)\s*\(([^)]*)\)", _header()):
        got = []
        for prm in [x.strip() for x in params.split(",") if x.strip() != "void"]:
            got.append("p" if "*" in prm else ("l" if prm.startswith("long") else "i"))
        assert got == [kinds[t] for t in _masslib.SIGNATURES[name]], name
    macros = {k: int(v) for k, v in re.findall(r"#define (DVAE_MASS_\w+) (\d+)", _header())}
    mirrored = {"DVAE_MASS_VERSION": _masslib.VERSION, "DVAE_MASS_MAX_FACTORS": _masslib.MAX_FACTORS, "DVAE_MASS_MAX_BINS": _masslib.MAX_BINS,
                "DVAE_MASS_WAVE_BINS": _masslib.WAVE_BINS, "DVAE_MASS_BLOCK_ROWS": _masslib.BLOCK_ROWS,
                "DVAE_MASS_MAX_CHUNKS": _masslib.MAX_CHUNKS, "DVAE_MASS_TRIP_ROWS": _masslib.TRIP_ROWS,
                "DVAE_MASS_LDS_DOUBLES": _masslib.LDS_DOUBLES}
    assert macros == mirrored                                            # every macro of the header, none besides
    assert _masslib.MAX_BINS >= 256 and _masslib.MAX_FACTORS == _infolib.MAX_FACTORS == 8
    assert _masslib.lib().dvae_mass_version() == _masslib.VERSION == 1
    binding = open(_masslib.__file__).read()
    assert 'Binding.for_library("mass", SIGNATURES, _RESTYPE' in binding and "LIB_PATH = _binding.path" in binding
    assert _masslib._binding.last_error == "dvae_mass_last_error" and _masslib._binding.signatures is _masslib.SIGNATURES
    assert _masslib._binding.soname == "libdvae_mass_hip.so"
    monkeypatch.setenv("DVAE_MASS_HIP_LIB", "/elsewhere/lib.so")            # the override, read when a binding is made
    assert _cabi.Binding.for_library("mass", {}, {}, "", subdir="ext").path == "/elsewhere/lib.so"
    monkeypatch.delenv("DVAE_MASS_HIP_LIB")
    # the sub-directory is optional: the calls of the other eleven bindings keep their paths
    assert os.path.normpath(_cabi.Binding.for_library("sep", {}, {}, "").path).endswith(os.path.join("lib", "libdvae_sep_hip.so"))
    assert os.path.normpath(_cabi.Binding.for_library("mass", {}, {}, "", "ext").path).endswith(os.path.join("lib", "ext", "libdvae_mass_hip.so"))
    for name in ("interpretability_scores_from_table", "interpretability_scores_from_mass"):
        assert name in disvae_amd.__all__ and getattr(disvae_amd, name) is getattr(E, name)
    # the limits the issue of this feature sets: dSprites unsplit, Cars3D's 183-valued factor accepted (two column groups)
    assert _masslib.column_groups(100, sum((3, 6, 40, 32, 32))) == (1, 113)
    assert 100 * 183 <= _masslib.LDS_DOUBLES and 8 * _masslib.LDS_DOUBLES <= 160 * 1024
    assert _masslib.column_groups(100, sum((4, 24, 183))) == (2, 106)
    # the chunk cap is cheap to reach: a few ten thousand rows
    assert _masslib.BLOCK_ROWS * _masslib.MAX_CHUNKS <= 40000 and _masslib.TRIP_ROWS < _masslib.BLOCK_ROWS


def test_build_has_the_fourth_list_and_the_other_three_are_unchanged():
    build = _build()
    assert [tuple(row) for row in build.EXTRA_TARGETS] == [("mass", ["posterior_mass"], "dvae_mass_hip.h")]
    assert [tuple(row) for row in build.SCORE_PLUGIN_TARGETS] == [("sep", ["latent_loo"], "dvae_sep_hip.h")]
    assert [tuple(row) for row in build.PLUGIN_TARGETS] == [("mmd", ["mmd_pairs"], "dvae_mmd_hip.h")]
    assert [n for n, _s, _h in build.TARGETS] == ["", "eval", "score", "info", "irs", "unsup", "udr", "dci", "dip"]
    assert "posterior_mass" not in build.ALL_SOURCES and len(build.ALL_SOURCES) == 31
    assert "posterior_mass" not in open(os.path.join(ROOT, "tools", "isa_identity.py")).read()
    assert build.MASS_SOURCES == ["posterior_mass"] and os.path.exists(os.path.join(build.SRC, SOURCE))
    lib_dir = os.path.join(ROOT, "disentangling-vae_amd", "lib")
    assert os.path.abspath(build.MASS_LIB) == os.path.join(lib_dir, "ext", "libdvae_mass_hip.so") and os.path.exists(build.MASS_LIB)
    assert os.path.abspath(build.MASS_LIB) == os.path.abspath(_masslib.LIB_PATH)
    assert os.path.abspath(build.SEP_LIB) == os.path.join(lib_dir, "libdvae_sep_hip.so")          # no sub-directory: as before
    assert os.path.abspath(build.LIB) == os.path.join(lib_dir, "libdvae_hip.so")
    assert sorted(os.path.basename(h) for h in build.MASS_HEADERS if "include" in h.split(os.sep)) == ["dvae_hip.h", "dvae_mass_hip.h"]
    assert {os.path.basename(h) for h in build.MASS_HEADERS} - {"dvae_hip.h", "dvae_mass_hip.h"} == \
        {f for f in os.listdir(CSRC) if f.endswith(".h")}
    assert build._target(*build.EXTRA_TARGETS[0], subdir=build.EXTRA_DIR)[3] == os.path.join(build.OBJ, "flags_mass.txt")
    assert os.path.exists(os.path.join(build.OBJ, "flags_mass.txt"))         # build() stamped it: the same flags and stamp logic
    assert open(os.path.join(build.OBJ, "flags_mass.txt")).read() == open(os.path.join(build.OBJ, "flags_sep.txt")).read().replace(
        "latent_loo", "posterior_mass")
    twelve = [f for d, _dirs, files in os.walk(lib_dir) for f in files if re.fullmatch(r"libdvae(_\w+)?_hip\.so", f)]
    assert len(twelve) == 12 and len(set(twelve)) == 12, sorted(twelve)
    assert [f for f in os.listdir(os.path.join(lib_dir, "ext")) if f.endswith(".so")] == ["libdvae_mass_hip.so"]
    src = open(os.path.join(CSRC, SOURCE)).read()
    assert sorted(re.findall(r'^#include "([^"]+)"', src, re.M)) == ["../../include/dvae_mass_hip.h", "common.h", "last_error.h",
                                                                     "table_stats.h"]


def test_source_obeys_the_rules_of_the_score_libraries():
    src = open(os.path.join(CSRC, SOURCE)).read()
    assert len(re.findall(r'^#include "last_error\.h"', src, re.M)) == 1
    assert not re.search(r"\bthread_local\b", src) and not re.search(r"^void set_error\(", src, re.M)
    for name in ("put_f64", "get_f64", "chunks_of", "lesser"):              # table_stats.h is their one home
        assert not re.search(r"^[ \w]*\b(?:void|double|int|T)\s+%s\s*\([^;{]*\)\s*\{" % name, src, re.M), name
    code = re.sub(r"//[^\n]*", "", src.split("#include", 1)[1])
    assert not re.search(r"atomic", code)                                   # no atomics of any kind
    assert "while" not in code and "hipLaunchCooperativeKernel" not in src  # no spinning, no cooperative launch
    assert not re.search(r"hipMalloc|hipFree|hipMemcpy|hipMemset|Synchronize", src)    # the entry points only enqueue
    # the numerical rule: one erfc, of |t|; no erf, no Phi(b) - Phi(a)
    assert len(re.findall(r"\berfc\(", code)) == 1 and "erfc(fabs(tj))" in code and not re.search(r"\berf\(", code)


def _put(good, i, v):
    return good[:i] + [v] + good[i + 1:]


def test_bad_arguments_are_refused_before_a_launch_with_the_librarys_own_text():
    h = _masslib.lib()
    assert h is _masslib.lib()                                             # loaded once
    bad = [_put(JOINT, i, None) for i in (0, 1, 3, 4, 11, 12)]             # (rows may be NULL; edges only with one bin)
    bad += [_put(JOINT, 5, 0), _put(JOINT, 5, -1), _put(JOINT, 6, 0), _put(JOINT, 6, -1), _put(JOINT, 6, 16385)]
    bad += [_put(JOINT, 7, 0), _put(JOINT, 7, _masslib.MAX_FACTORS + 1), _put(JOINT, 8, 0), _put(JOINT, 8, -3)]
    bad += [_put(JOINT, 9, 0), _put(JOINT, 9, -1), _put(JOINT, 9, _masslib.MAX_BINS + 1), _put(JOINT, 10, 1), _put(JOINT, 10, 0)]
    bad += [_put(_put(JOINT, 6, 16384), 10, 2 ** 31 // (8 * 16384) + 1)]    # D * n_bins * sum_sizes past 2^31 - 1
    for args in bad:
        with pytest.raises(_lib.DvaeHipError) as e:
            _masslib.call("dvae_mass_joint", *args)
        own = h.dvae_mass_last_error().decode()
        assert "invalid argument" in own and SOURCE in own, (args, own)
        assert str(e.value) == "dvae_mass_joint failed (-1): %s" % own
    with pytest.raises(_lib.DvaeHipError, match=r"n_bins >= 1 && n_bins <= DVAE_MASS_MAX_BINS"):     # the range, in the library's own words
        _masslib.call("dvae_mass_joint", *_put(JOINT, 9, _masslib.MAX_BINS + 1))
    with pytest.raises(_lib.DvaeHipError, match=r"edges \|\| n_bins == 1"):
        _masslib.call("dvae_mass_joint", *_put(JOINT, 4, None))
    assert SOURCE not in _infolib.lib().dvae_info_last_error().decode()    # every library keeps its own buffer


def test_call_loads_through_the_modules_lib(monkeypatch):
    class Boom(Exception):
        pass

    def boom():
        raise Boom("lib() of the module was asked")
    monkeypatch.setattr(_masslib, "lib", boom)
    with pytest.raises(Boom, match="was asked"):
        _masslib.call("dvae_mass_joint", *JOINT)


def test_workspace_size_mirrors_its_python_twin_and_is_zero_out_of_range():
    ws = _masslib.lib().dvae_mass_ws_doubles
    for args in ((0, 3, 2, 4, 8, 5), (6, 0, 2, 4, 8, 5), (6, 3, 0, 4, 8, 5), (6, 3, 9, 4, 8, 9), (6, 3, 2, 4, 0, 5), (6, 3, 2, 4, 257, 5),
                 (6, 3, 2, 4, 8, 1), (-1, 3, 2, 4, 8, 5), (6, 16385, 2, 4, 8, 5), (6, 16384, 2, 4, 8, 2 ** 31 // (8 * 16384) + 1),
                 (0, 3, 2, 0, 8, 5)):
        assert ws(*args) == _masslib.ws_doubles(*args) == 0, args
    cap = _masslib.BLOCK_ROWS * _masslib.MAX_CHUNKS
    for S in (1, 63, 64, 65, 255, 256, 257, 10000, cap - 1, cap, cap + 1, 2 * cap + 1, 737280):
        for D, K, nb, sums in ((1, 3, 4, 9), (10, 5, 100, 113), (17, 2, 256, 79), (3, 1, 1, 2)):
            want = _masslib.chunks(S)[0] * D * nb * sums
            assert ws(737280, D, K, S, nb, sums) == _masslib.ws_doubles(737280, D, K, S, nb, sums) == want, (S, D, nb)
        n, rows = _masslib.chunks(S)
        assert n <= _masslib.MAX_CHUNKS and n * rows >= S > (n - 1) * rows and (S > cap or rows <= _masslib.BLOCK_ROWS)
    assert ws(737280, 10, 5, 0, 100, 113) == ws(737280, 10, 5, 737280, 100, 113)           # S <= 0: as for NULL rows
    assert _masslib.chunks(cap) == (_masslib.MAX_CHUNKS, _masslib.BLOCK_ROWS) and _masslib.chunks(cap + 1) == (_masslib.MAX_CHUNKS, _masslib.BLOCK_ROWS + 1)
    assert ws(737280, 10, 5, 737280, 100, 113) * 8 < 1 << 27                               # the dSprites shape: under 128 MiB
    # the column split: one group while the accumulators fit, then as few as fit, the columns spread evenly
    fit = _masslib.LDS_DOUBLES // _masslib.MAX_BINS
    assert _masslib.column_groups(_masslib.MAX_BINS, fit) == (1, fit) and _masslib.column_groups(_masslib.MAX_BINS, fit + 1) == (2, (fit + 2) // 2)
    for nb in (1, 4, 100, 256):
        for sums in (2, 78, 79, 200, 201, 1000, 20001):
            groups, cols = _masslib.column_groups(nb, sums)
            assert cols * nb <= _masslib.LDS_DOUBLES and groups * cols >= sums > (groups - 1) * cols


# ---- 2. the restatement ------------------------------------------------------------------------------------------------------------
def test_restatement_against_scipy_and_mpmath_pins_u_ref():
    special = pytest.importorskip("scipy.special")
    mpmath = pytest.importorskip("mpmath")
    t = R.erfc_arguments(CASES)
    assert 10000 <= len(t) <= 40000 and (t < 0).any() and (np.abs(t) > 20).any() and (np.abs(t) < 1e-3).any()
    ours = np.array([math.erfc(x) for x in t])
    theirs = special.erfc(t)
    normal = ours > 1e-300                                              # (below: the subnormals, and 0 from |t| = 27 on in both)
    assert (np.abs(ours - theirs)[normal] <= 2e-13 * theirs[normal]).all()    # (scipy's own error grows with t^2: 5e-14 at t = 23)
    assert (theirs[~normal] <= 1e-300).all() and normal.sum() > len(t) // 2
    worst, at = 0.0, None
    with mpmath.workprec(140):                                           # 40 digits and more
        for x, got in zip(t, ours):
            true = mpmath.erfc(mpmath.mpf(float(x)))
            if true < 1e-300:
                continue
            err = abs(float((mpmath.mpf(float(got)) - true) / float(np.spacing(float(true)))))
            if err > worst:
                worst, at = err, float(x)
    print("math.erfc against mpmath over %d arguments: worst %.3f ulp at t = %r; U_REF = %g" % (len(t), worst, at, R.U_REF))
    assert worst <= R.U_REF and R.U_REF == 3.0
    # row_masses (the definition, one bin at a time) and masses (vectorised) are the same numbers; mpmath agrees to the bound
    mean, logvar = R.table("edge", 12, 2, 100, seed=5)
    e = R.edges(100)
    Q = R.masses(mean, logvar, e)
    for r in range(12):
        for d in range(2):
            np.testing.assert_allclose(Q[r, d], R.row_masses(mean[r, d], logvar[r, d], e), rtol=1e-13, atol=2.0 ** -52)   # (exp: numpy's or libm's)
    with mpmath.workprec(140):
        for r, d in ((0, 0), (5, 1), (11, 0)):
            s = mpmath.exp(mpmath.mpf(float(logvar[r, d])) / 2) * mpmath.sqrt(2)
            cdf = [mpmath.mpf(0)] + [1 - mpmath.erfc((mpmath.mpf(float(x)) - mpmath.mpf(float(mean[r, d]))) / s) / 2 for x in e] + [mpmath.mpf(1)]
            true = np.array([float(cdf[b + 1] - cdf[b]) for b in range(100)])
            assert np.abs(Q[r, d] - true).max() <= (2 * R.U_REF + 3) * 2.0 ** -53
            big = true > 1e-300
            assert (np.abs(Q[r, d] - true)[big] <= 1e-9 * true[big]).all()     # small cells keep their digits


def test_tail_difference_rule():
    mean, logvar = R.far_sharp_table()
    assert mean.shape == (1440, 1) and np.abs(mean).max() > 30 and logvar.min() < -13.9
    e = R.edges(100)
    Q, Qerf = R.masses(mean, logvar, e), R.masses_erf_form(mean, logvar, e)
    sums = np.abs(Q.sum(axis=2) - 1.0).max()
    cells = Q > 1e-30
    rel = np.abs(Qerf - Q)[cells] / Q[cells]
    print("row sums within %.2f x 2^-53 of 1; erf form: worst relative error %.3g on cells above 1e-30, %d of %d at 0.5 or more"
          % (sums / 2.0 ** -53, rel.max(), (rel >= 0.5).sum(), cells.sum()))
    assert (Q >= 0).all() and sums <= 4 * 2.0 ** -53 * 100
    assert rel.max() >= 0.5
    assert np.abs(Qerf.sum(axis=2) - 1.0).max() <= 1e-15                  # ... and its row sums do not show it


def test_restatement_pieces():
    assert R.edges(4).tolist() == [-2.0, 0.0, 2.0] and len(R.edges(1)) == 0 and np.array_equal(R.edges(100), E.mass_edges(100))
    assert np.array_equal(R.edges(7, (-1.0, 2.5)), np.linspace(-1.0, 2.5, 8)[1:-1]) and R.edges(100).dtype == np.float64
    assert R.factor_values([0, 1, 5, 23], (4, 3, 2)).tolist() == [[0, 0, 0], [0, 0, 1], [0, 2, 1], [3, 2, 1]]
    assert R.row_masses(0.3, -2.0, R.edges(1)).tolist() == [1.0]
    q = R.row_masses(0.0, 0.0, R.edges(2))
    assert q.tolist() == [0.5, 0.5]                                       # the mean on the one edge
    mean, logvar = R.table("broad", 24, 2, 4, seed=1)
    rows = np.array([3, 3, 7, 23, 0, 3])
    mass, n_v = R.mass_table(mean, logvar, (4, 3, 2), 4, rows=rows)
    assert mass.shape == (2, 4 * 9) and n_v.tolist() == [4, 1, 0, 1, 2, 3, 1, 1, 5]
    Q = R.masses(mean, logvar, R.edges(4))
    block = mass[1, 4 * 4:4 * 7].reshape(4, 3)                             # latent 1, factor 1
    np.testing.assert_allclose(block[:, 1], 3 * Q[3, 1], rtol=1e-15)
    assert np.array_equal(block[:, 0], Q[7, 1] + Q[0, 1]) and np.array_equal(block[:, 2], Q[23, 1])      # in the order of `rows`
    assert R.cell_counts(n_v, (4, 3, 2), 4).reshape(-1)[:8].tolist() == [4, 1, 0, 1, 4, 1, 0, 1]


# ---- 3. the scores from hand-made mass tables -----------------------------------------------------------------------------------
def _table_of(blocks):
    """blocks[d][k]: [n_bins, size_k] -> mass [D, n_bins * sum sizes]."""
    return np.stack([np.concatenate([np.asarray(b, dtype=np.float64).reshape(-1) for b in row]) for row in blocks])


def _assert_matches_restatement(got, mass, lat_sizes, n_bins):
    want = R.scores(mass, lat_sizes, n_bins)
    assert set(got) == set(want) | {"n_samples", "n_bins"}
    for k, v in want.items():
        np.testing.assert_allclose(got[k], v, rtol=1e-12, atol=1e-12, err_msg=k)
    assert got["mutual_information"].shape == got["joint_entropy"].shape == (mass.shape[0], len(lat_sizes))
    assert all(isinstance(got[k], float) for k in R.SCALAR_SCORES) and got["n_bins"] == n_bins
    json.dumps({k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in got.items()})


def test_scores_of_a_permutation_table():
    """Latent k holds factor k, one bin per value, the other latents' masses independent of every factor."""
    sizes, nb = (3, 2), 4
    perm0, perm1 = np.zeros((nb, 3)), np.zeros((nb, 2))
    perm0[[2, 0, 3], [0, 1, 2]] = 4.0                                     # 12 rows: 4 per value of factor 0, 6 per value of factor 1
    perm1[[1, 3], [0, 1]] = 6.0
    flat0, flat1 = np.full((nb, 3), 1.0), np.full((nb, 2), 1.5)
    mass = _table_of([[perm0, flat1], [flat0, perm1], [flat0, flat1]])
    got = E.interpretability_scores_from_mass(mass, sizes, nb)
    _assert_matches_restatement(got, mass, sizes, nb)
    assert got["n_samples"] == 12 and got["best_latent"].tolist() == [0, 1]
    np.testing.assert_allclose(got["factor_entropy"], np.log([3, 2]), rtol=1e-15)
    np.testing.assert_allclose(got["mutual_information"], [[math.log(3), 0], [0, math.log(2)], [0, 0]], atol=1e-15)
    assert got["rmig_norm"] == pytest.approx(1.0, abs=1e-15) and got["dcimig"] == pytest.approx(1.0, abs=1e-15)
    assert got["mig_sup"] == pytest.approx(2.0 / 3.0, abs=1e-15)
    H, I = got["joint_entropy"], got["mutual_information"]
    assert got["jemmig_per_factor"].tolist() == [H[0, 0] - I[0, 0], H[1, 1] - I[1, 1]]          # exactly: the runner-up's MI is 0
    np.testing.assert_allclose(got["jemmig_per_factor"], 0.0, atol=1e-15)                       # one bin per value: nothing besides
    np.testing.assert_allclose(got["jemmig_norm_per_factor"], 1.0, atol=1e-15)
    np.testing.assert_allclose(got["latent_entropy"], [math.log(3), math.log(4), math.log(4)], rtol=1e-15)


def test_scores_of_an_independent_table_and_the_ties():
    sizes, nb = (3, 2), 4
    pz = np.array([0.1, 0.2, 0.3, 0.4])
    flat0, flat1 = 12 * np.outer(pz, [1 / 3] * 3), 12 * np.outer(pz, [0.5] * 2)
    mass = _table_of([[flat0, flat1], [flat0, flat1]])
    got = E.interpretability_scores_from_mass(mass, sizes, nb)
    _assert_matches_restatement(got, mass, sizes, nb)
    for k in ("rmig", "rmig_norm", "mig_sup", "dcimig"):
        assert abs(got[k]) <= 1e-15, k
    assert got["best_latent"].tolist() == [0, 0]                          # ties: the lowest d
    # two latents that hold factor 0 equally well: the lowest wins, the gap is 0, JEMMIG pays for the runner-up
    perm0 = np.zeros((nb, 3))
    perm0[[2, 0, 3], [0, 1, 2]] = 4.0
    mass = _table_of([[flat0, flat1], [perm0, flat1], [perm0, flat1]])
    got = E.interpretability_scores_from_mass(mass, sizes, nb)
    _assert_matches_restatement(got, mass, sizes, nb)
    assert got["best_latent"].tolist() == [1, 0] and got["rmig_per_factor"][0] == 0.0
    assert got["jemmig_per_factor"][0] == got["joint_entropy"][1, 0]
    # D = 1 and K = 1: the runner-up is 0 in both branches
    one = E.interpretability_scores_from_mass(_table_of([[perm0]]), (3,), nb)
    _assert_matches_restatement(one, _table_of([[perm0]]), (3,), nb)
    assert one["best_latent"].tolist() == [0] and one["rmig_norm"] == pytest.approx(1.0, abs=1e-15)
    assert one["mig_sup_per_latent"].tolist() == [one["mutual_information"][0, 0] / one["factor_entropy"][0]]
    assert one["dcimig"] == pytest.approx(1.0, abs=1e-15)
    two = E.interpretability_scores_from_mass(_table_of([[perm0], [perm0]]), (3,), nb)         # K = 1, a tie over d
    assert two["best_latent"].tolist() == [0] and two["rmig"] == 0.0 and two["dcimig"] == pytest.approx(1.0, abs=1e-15)


def test_a_factor_without_entropy_raises_and_the_shape_is_checked():
    nb = 4
    const = np.zeros((nb, 3))
    const[:, 1] = 3.0                                                     # every selected row carries value 1
    with pytest.raises(ValueError, match=r"factor\(s\) \[0\] take one value among the selected rows"):
        E.interpretability_scores_from_mass(_table_of([[const, np.full((nb, 2), 1.5)]]), (3, 2), nb)
    with pytest.raises(ValueError, match=r"mass must be \[D, n_bins \* sum\(lat_sizes\)\]"):
        E.interpretability_scores_from_mass(np.ones((2, 19)), (3, 2), nb)


def test_masses_of_1e_minus_300_give_finite_scores_without_a_warning():
    """Sharp posteriors leave cells of 1e-300 and less beside cells of 1: the product of two such marginals underflows where the
    cell itself has not, so the ratio under the logarithm is formed as (P / P_z) / P_v."""
    import warnings
    mean, _ = R.ideal_table()
    mass, _n_v = R.mass_table(mean, np.full_like(mean, -12.0), R.GRID, 100)
    assert ((mass > 0) & (mass < 1e-300)).any()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = E.interpretability_scores_from_mass(mass, R.GRID, 100)
    _assert_matches_restatement(got, mass, R.GRID, 100)
    assert all(math.isfinite(got[k]) for k in R.SCALAR_SCORES) and got["rmig_norm"] >= 0.99


# ---- 4. the thresholds of the end-to-end GPU test, on the reference alone -----------------------------------------------------------
def test_thresholds_of_the_ideal_and_the_rotated_table():
    assert R.GRID == (6, 5, 4, 3, 2)
    got = {}
    for name, (mean, logvar) in (("ideal", R.ideal_table()), ("rotated", R.rotated_table())):
        assert mean.shape == logvar.shape == (720, 7) and mean.dtype == logvar.dtype == np.float32
        mass, n_v = R.mass_table(mean, logvar, R.GRID, 100)
        np.testing.assert_allclose(mass.reshape(7, -1).sum(axis=1), 5 * 720, rtol=1e-13)       # every row, once per factor
        got[name] = s = E.interpretability_scores_from_mass(mass, R.GRID, 100)
        _assert_matches_restatement(s, mass, R.GRID, 100)
        print("%s: %s" % (name, {k: round(s[k], 4) for k in R.SCALAR_SCORES}))
    assert got["ideal"]["rmig_norm"] >= 0.99 and got["ideal"]["jemmig_norm"] >= 0.9
    assert got["rotated"]["rmig_norm"] <= 0.5 and got["rotated"]["jemmig_norm"] <= 0.35
    assert got["ideal"]["best_latent"].tolist() == [0, 1, 2, 3, 4] and got["ideal"]["dcimig"] >= 0.99
    # the two collapsed latents tell nothing: a discretised MIG of their MEANS could not know that they are as wide as the range
    assert got["ideal"]["mutual_information"][5:].max() <= 1e-3 and got["ideal"]["mig_sup_per_latent"][5:].max() <= 1e-3


# ---- 5. errors before any library call -------------------------------------------------------------------------------------------
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


class _Model(torch.nn.Module):
    latent_dim = 2

    def __init__(self):
        super().__init__()
        self.modes = []

    def encoder(self, x):
        self.modes.append(self.training)
        return torch.zeros(x.shape[0], 2), torch.zeros(x.shape[0], 2)


def test_argument_errors_raise_before_any_library_call(monkeypatch):
    def no_library():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_masslib, "lib", no_library)
    mean, logvar = torch.zeros(6, 4), torch.zeros(6, 4)
    top = _masslib.MAX_BINS
    for sizes, kw, msg in (([3, 3], {}, "does not enumerate"), ([3, 2], dict(n_bins=0), r"n_bins must lie in \[1, %d\]" % top),
                           ([3, 2], dict(n_bins=top + 1), r"n_bins must lie in \[1, %d\]" % top), ([6, 1], {}, "one value"),
                           ([1] * 8 + [6], {}, "at most 8"), ([3, 2], dict(n_samples=7), r"n_samples must lie in \[1, 6\]"),
                           ([3, 2], dict(n_samples=0), r"n_samples must lie in \[1, 6\]"), ([3, 2], dict(rows=[0, 6]), r"in \[0, 6\)"),
                           ([3, 2], dict(rows=[]), "one row number or more"), ([0, 2], {}, "positive sizes"),
                           ([3, 2], dict(z_range=(1.0, 1.0)), "z_range must be"), ([3, 2], dict(z_range=(-4.0, float("inf"))), "z_range must be"),
                           ([3, 2], dict(z_range=(2.0, -2.0)), "z_range must be"), ([3, 2], dict(z_range=(1.0,)), "z_range must be")):
        with pytest.raises(ValueError, match=msg):
            E.interpretability_scores_from_table(mean, logvar, sizes, **kw)
    with pytest.raises(ValueError, match="table"):
        E.interpretability_scores_from_table(torch.zeros(6), torch.zeros(6), [3, 2])
    with pytest.raises(ValueError, match="logvar must have the shape of mean"):
        E.interpretability_scores_from_table(mean, torch.zeros(6, 3), [3, 2])
    for which in (0, 1):
        bad = [mean.clone(), logvar.clone()]
        bad[which][4, 1] = float("nan") if which else float("inf")
        with pytest.raises(ValueError, match="NaN or an infinity"):
            E.interpretability_scores_from_table(bad[0], bad[1], [3, 2])
    with pytest.raises(_lib.DvaeHipError, match="no CPU"):
        E.interpretability_scores_from_table(mean, logvar, [3, 2])
    model = _Model().train()
    ev = E.Evaluator(model, None, is_progress_bar=False)
    with pytest.raises(ValueError, match="known true factors"):
        ev.compute_interpretability_scores(_Loader([0, 1, 2], None))
    for kw, msg in ((dict(n_bins=top + 1), "n_bins must lie"), (dict(n_samples=7), "n_samples must lie"), (dict(z_range=(0.0, 0.0)), "z_range")):
        with pytest.raises(ValueError, match=msg):
            ev.compute_interpretability_scores(_Loader(_Factors(6), None), **kw)
    with pytest.raises(ValueError, match=r"data set of 5 images does not enumerate lat_sizes=\[3, 2\]"):
        ev.compute_interpretability_scores(_Loader(_Factors(5), None))
    assert model.modes == [] and model.training
    loader = _Loader(_Factors(6), [(torch.rand(4, 1), None), (torch.rand(2, 1), None)])
    with pytest.raises(_lib.DvaeHipError, match="no CPU"):                 # valid arguments: the table is on the CPU
        ev.compute_interpretability_scores(loader)
    assert model.modes == [False, False] and model.training               # encoded in eval mode, and the mode is as it was


def test_call_writes_the_interpretability_scores_on_request(monkeypatch, tmp_path):
    seen = []
    model = _Model().train()
    ev = E.Evaluator(model, None, is_progress_bar=False, save_dir=str(tmp_path))
    result = {"rmig": 0.5, "rmig_per_factor": np.array([0.25, 0.75]), "best_latent": np.array([1, 0]), "mutual_information": np.ones((2, 2)),
              "joint_entropy": np.ones((2, 2)), "n_samples": 11, "n_bins": 100}
    monkeypatch.setattr(ev, "compute_interpretability_scores", lambda loader, **kw: seen.append((loader, kw, model.training)) or result)
    monkeypatch.setattr(ev, "compute_losses", lambda loader: {"loss": 1.5})
    loader = object()
    assert ev(loader) == (None, {"loss": 1.5}) and seen == [] and os.listdir(tmp_path) == ["test_losses.log"]
    assert ev(loader, is_losses=False, is_interpretability=True) == (None, None)
    assert seen == [(loader, {}, False)] and model.training
    assert ev(loader, is_losses=False, is_interpretability=True, interpretability_args=dict(n_samples=11, n_bins=50)) == (None, None)
    assert seen[-1] == (loader, dict(n_samples=11, n_bins=50), False)
    assert E.INTERPRETABILITY_SCORES_FILE == "interpretability_scores.log"
    assert json.load(open(tmp_path / "interpretability_scores.log")) == {"rmig": 0.5, "rmig_per_factor": [0.25, 0.75], "best_latent": [1, 0],
                                                                          "n_samples": 11, "n_bins": 100}       # without the [D, K] matrices
