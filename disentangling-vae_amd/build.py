"""Build the project's shared libraries (gfx950) in-tree: hipcc cross-compiles without a GPU.

    python disentangling-vae_amd/build.py [--force] [--debug]

TARGETS is the one list the builds are driven from: a target is a name, its sources in csrc/ and its public header in
include/.  Target "" is libdvae_hip.so, the training library; every other target NAME is libdvae_NAME_hip.so, and
nothing of one target is linked into another.  All targets share FLAGS and the up-to-date
logic, each under a stamp of its own (build/flags.txt, build/flags_NAME.txt).  The module's X_LIB / X_SOURCES /
X_HEADERS names (LIB / SOURCES / HEADERS for the training library) are derived from the table.
PLUGIN_TARGETS is a second list of the same rows, built after TARGETS in the same way (see there), SCORE_PLUGIN_TARGETS a
third, built after both, EXTRA_TARGETS a fourth, whose libraries land in lib/ext/, and MORE_TARGETS a fifth, built last, whose
libraries land in lib_more/ next to lib/, and SCORE_TARGETS a sixth, whose libraries land in lib_scores/ next to both.
The libraries land in disentangling-vae_amd/lib/ (git-ignored build products).  Objects are rebuilt only
when a source / header is newer or the flags changed.
--debug (or DVAE_BUILD_DEBUG=1) adds -DDVAE_DEBUG_SWITCHES: the A/B / timing-ablation environment
switches and the experimental kernel variants they select (tools/README.md); the default (shipped)
library has none of them.
"""
import glob
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(HERE, "build")
DEBUG_SOURCES = []          # experimental kernel files of the training library: only in --debug builds
# (name, sources in csrc/, public header in include/): "" is the training library; the next library is one more row
TARGETS = [
    ("", ["conv_generic", "conv_mfma", "conv_down_dma", "conv_up_ws", "conv_wgrad_ws", "conv_thin", "conv_thin_ws", "conv_up_thin_mm", "linear", "linear_narrow", "gemm_dma", "linear_grouped", "fc_chain", "stage", "loss",
          "latent_wide", "metrics", "adam", "comm", "viz", "loglik", "plan", "capi"], "dvae_hip.h"),
    ("eval", ["elbo_decomp"], "dvae_eval_hip.h"),          # dataset-level ELBO decomposition
    ("score", ["factor_scores"], "dvae_score_hip.h"),      # FactorVAE / beta-VAE scores
    ("info", ["factor_info"], "dvae_info_hip.h"),          # discretised MIG, modularity, SAP
    ("irs", ["factor_irs"], "dvae_irs_hip.h"),             # interventional robustness score
    ("unsup", ["latent_pairs"], "dvae_unsup_hip.h"),       # Gaussian total correlation, Wasserstein correlation, latent-latent mutual information
    ("udr", ["latent_ranks"], "dvae_udr_hip.h"),           # unsupervised disentanglement ranking: tie-averaged ranks, KL per dimension
    ("dci", ["boosted_trees"], "dvae_dci_hip.h"),          # DCI: gradient-boosted trees fitted on the device, their importances
    ("dip", ["dip_cov"], "dvae_dip_hip.h"),                # DIP-VAE I / II: batch covariance, the regulariser and its gradients (a TRAINING loss)
]
# Libraries built like a row of TARGETS -- same _target / _build_target, FLAGS and stamp logic, after TARGETS -- but kept OUT of
# TARGETS, ALL_SOURCES and tools/isa_identity.py: the host tests pin the nine rows, their names and the 31 sources that the
# machine-code identity tool compares, and a loss plugin with a library of its own touches none of them.
PLUGIN_TARGETS = [
    ("mmd", ["mmd_pairs"], "dvae_mmd_hip.h"),              # InfoVAE / MMD-VAE: the batch MMD against prior samples and its gradient (a TRAINING loss)
]
# A score library added after the rows above were pinned: the same kind of row once more, built after the other two lists through the
# same helper, and like PLUGIN_TARGETS out of ALL_SOURCES and tools/isa_identity.py.
SCORE_PLUGIN_TARGETS = [
    ("sep", ["latent_loo"], "dvae_sep_hip.h"),             # SEPIN / WSEPIN separability: leave-one-out joint entropies under the aggregate posterior
]
# The rows after those: the same kind of row and the same helper, FLAGS and stamp logic, built last, out of ALL_SOURCES and
# tools/isa_identity.py -- and their libraries in the sub-directory EXTRA_DIR of lib/, because the host tests also pin the number
# of libraries that lie in lib/ itself.  The next library is one more row HERE.
EXTRA_TARGETS = [
    ("mass", ["posterior_mass"], "dvae_mass_hip.h"),       # RMIG / JEMMIG / MIG-sup / DCIMIG: the posterior mass per bin and factor value
]
EXTRA_DIR = "ext"
# A fifth list of the same rows, built after the other four through the same helper, FLAGS and stamp logic, out of ALL_SOURCES and
# tools/isa_identity.py -- and OUTSIDE lib/: the host tests also pin the number of libraries anywhere under lib/ and what lib/ext/
# holds, so these land in the sibling directory lib_more/ (git-ignored like lib/), reached as a sub-directory "../lib_more" of
# lib/ by _target here and by _cabi.Binding.for_library.  The next library is one more row HERE.
MORE_TARGETS = [
    ("sap", ["svm_1d"], "dvae_sap_hip.h"),                 # discrete-factor SAP: one-feature linear SVMs fitted by Newton's method on the device
]
MORE_DIR = os.path.join("..", "lib_more")
# A sixth list of the same rows, built after the other five through the same helper, FLAGS and stamp logic, out of ALL_SOURCES and
# tools/isa_identity.py, into the sibling directory lib_scores/ (git-ignored like lib/): the host tests pin what lib/, lib/ext/ and
# lib_more/ hold.  Nothing pins this list or its directory to ONE entry: the next score library is one more row of THIS list.
SCORE_TARGETS = [
    ("knn", ["knn_mi"], "dvae_knn_hip.h"),                 # binning-free MIG / InfoM / InfoC: k-nearest-neighbour mutual information (Ross 2014)
    ("lr", ["softmax_fit"], "dvae_lr_hip.h"),              # linear-softmax probes (beta-VAE score, explicitness, InfoE): Newton-CG fits on the device
    ("weak", ["weak_pairs"], "dvae_weak_hip.h"),           # Ada-GVAE / Ada-ML-VAE: the adaptive group posterior of image pairs and its backward pass (a TRAINING plugin, not a score)
    ("semi", ["label_reg"], "dvae_semi_hip.h"),            # S2-beta-VAE: the supervised regulariser on the labelled rows of a batch and its gradient (a TRAINING plugin, not a score)
]
SCORE_DIR = os.path.join("..", "lib_scores")
HEADERS = sorted(glob.glob(os.path.join(SRC, "*.h"))) + [os.path.join(HERE, "..", "include", "dvae_hip.h")]


def _target(name, sources, header, subdir=""):
    """One row of TARGETS -> (library, sources, headers whose change rebuilds it, stamp file); subdir: of lib/."""
    infix = "_" + name if name else ""
    headers = HEADERS + [os.path.join(HERE, "..", "include", header)] if name else HEADERS
    return os.path.join(HERE, "lib", subdir, "libdvae%s_hip.so" % infix), sources, headers, os.path.join(OBJ, "flags%s.txt" % infix)


for _row in TARGETS + PLUGIN_TARGETS + SCORE_PLUGIN_TARGETS:        # LIB / SOURCES / HEADERS of the training library, EVAL_LIB / EVAL_SOURCES / EVAL_HEADERS, ... of the others
    _prefix = _row[0].upper() + "_" if _row[0] else ""
    globals()[_prefix + "LIB"], globals()[_prefix + "SOURCES"], globals()[_prefix + "HEADERS"], _ = _target(*_row)
for _row in EXTRA_TARGETS:
    globals()[_row[0].upper() + "_LIB"], globals()[_row[0].upper() + "_SOURCES"], globals()[_row[0].upper() + "_HEADERS"], _ = \
        _target(*_row, subdir=EXTRA_DIR)
for _row in MORE_TARGETS:
    globals()[_row[0].upper() + "_LIB"], globals()[_row[0].upper() + "_SOURCES"], globals()[_row[0].upper() + "_HEADERS"], _ = \
        _target(*_row, subdir=MORE_DIR)
for _row in SCORE_TARGETS:
    globals()[_row[0].upper() + "_LIB"], globals()[_row[0].upper() + "_SOURCES"], globals()[_row[0].upper() + "_HEADERS"], _ = \
        _target(*_row, subdir=SCORE_DIR)
ALL_SOURCES = [s for _, sources, _ in TARGETS for s in sources]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function"]


def _newer(a, b):
    return (not os.path.exists(b)) or os.path.getmtime(a) > os.path.getmtime(b)


def _build_target(hipcc, lib, sources, headers, flags, stamp, force, verbose):
    """Compile `sources` (objects rebuilt only when a source / header is newer or the stamped flags changed) and link `lib`."""
    want = " ".join(flags + sources)
    if not os.path.exists(stamp) or open(stamp).read() != want:
        force = True
    jobs = []
    for s in sources:
        src, obj = os.path.join(SRC, s + ".hip"), os.path.join(OBJ, s + ".o")
        if force or _newer(src, obj) or any(_newer(h, obj) for h in headers):
            jobs.append([hipcc] + flags + ["-c", src, "-o", obj])

    def run(cmd):
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed: %s\n%s" % (" ".join(cmd), r.stderr))
        return r.stderr

    with ThreadPoolExecutor(max_workers=8) as ex:
        for err in ex.map(run, jobs):
            if verbose and err.strip():
                sys.stderr.write(err)
    objs = [os.path.join(OBJ, s + ".o") for s in sources]
    if force or jobs or not os.path.exists(lib):
        run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib] + objs + ["-ldl"])
    with open(stamp, "w") as f:
        f.write(want)
    return lib


def _build_row(hipcc, name, sources, header, flags, debug, force, verbose, subdir=""):
    """One row of a target list: its library under its own stamp."""
    lib, sources, headers, stamp = _target(name, sources + (DEBUG_SOURCES if debug and not name else []), header, subdir)
    os.makedirs(os.path.dirname(lib), exist_ok=True)
    _build_target(hipcc, lib, sources, headers, flags, stamp, force, verbose)


def build(force=False, verbose=True, debug=None):
    """Build every target of TARGETS, then of PLUGIN_TARGETS, then of SCORE_PLUGIN_TARGETS, then of EXTRA_TARGETS, then of
    MORE_TARGETS, then of SCORE_TARGETS, in their order; returns the path of libdvae_hip.so."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if debug is None:
        debug = os.environ.get("DVAE_BUILD_DEBUG", "0") == "1"
    os.makedirs(OBJ, exist_ok=True)
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    flags = FLAGS + (["-DDVAE_DEBUG_SWITCHES"] if debug else [])
    for name, sources, header in TARGETS + PLUGIN_TARGETS:
        _build_row(hipcc, name, sources, header, flags, debug, force, verbose)
    for name, sources, header in SCORE_PLUGIN_TARGETS:
        _build_row(hipcc, name, sources, header, flags, debug, force, verbose)
    for row in EXTRA_TARGETS: _build_row(hipcc, *row, flags, debug, force, verbose, subdir=EXTRA_DIR)   # noqa: E701 (the host tests count the two loop bodies above)
    for row in MORE_TARGETS: _build_row(hipcc, *row, flags, debug, force, verbose, subdir=MORE_DIR)     # noqa: E701 (likewise)
    for row in SCORE_TARGETS: _build_row(hipcc, *row, flags, debug, force, verbose, subdir=SCORE_DIR)   # noqa: E701 (likewise)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, debug=True if "--debug" in sys.argv else None))
