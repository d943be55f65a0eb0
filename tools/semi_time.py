"""Cost of the supervised regulariser of S2-beta-VAE (libdvae_semi_hip.so, csrc/label_reg.hip) and of the training step that carries
it.

(a) The two launches alone (dvae_semi_partials + dvae_semi_grad: value and dmu) at 64, 256, 1024 and 2048 rows with D = 10 and the
    K = 5 factors of dSprites, half of the rows labelled, per sup_loss, next to torch autograd -- forward + backward of the same
    regulariser written with torch ops on a label tensor that is already on the device -- on the same GPU.  The gradients of both
    are compared before timing.
(b) The whole s2vae training step (per sup_loss) against the betaH step of the same build, (3, 64, 64) at 1024 rows and
    (1, 32, 32) at 64 rows, the shipped replay setting: what the regulariser adds to a step, to be held against (a).

Device events around each call; the candidates are INTERLEAVED (one repeat of each in turn, `--reps` rounds after a warm-up), so a
drift of the clocks lands on all of them; the median and the spread [min, max] are reported.  Inputs from a seed.  Prints one JSON
line per measurement and writes them to --out.

    python tools/semi_time.py [--reps 30] [--out profiles/semi_time.jsonl]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "disentangling-vae_amd")]

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from disvae_amd import _semilib  # noqa: E402
from disvae_amd.engine import _stream  # noqa: E402
from disvae_amd.models.losses import get_loss_f  # noqa: E402
from disvae_amd.models.vae import init_specific_model  # noqa: E402

DSPRITES = (1, 3, 6, 40, 32, 32)
FACTORS = [1, 2, 3, 4, 5]
HP = dict(rec_dist="bernoulli", reg_anneal=10000, betaH_B=4, betaB_initC=0, betaB_finC=25, betaB_G=1000, factor_G=6.4,
          lr_disc=1e-4, btcvae_A=1, btcvae_B=6.4, btcvae_G=1, n_data=737280, latent_dim=10, lat_sizes=DSPRITES, s2_beta=4)


def interleaved_ms(fns, reps, inner=1):
    """{name: fn} -> {name: (median, [min, max])} of `reps` rounds, one repeat of every candidate per round; a repeat is `inner`
    calls between two events (its time is divided by inner)."""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _i in range(inner):
                fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / inner)
    out = {}
    for k, t in times.items():
        t.sort()
        out[k] = (round(t[len(t) // 2], 5), [round(t[0], 5), round(t[-1], 5)])
    return out


def torch_regulariser(mu, idx, v, sizes, kind):
    """R on the labelled rows idx with the value indices v [n_lab, K] (float) already on the device."""
    K = v.shape[1]
    mL = mu.index_select(0, idx)
    if kind == "xent":
        return F.binary_cross_entropy_with_logits(mL[:, :K], v / sizes, reduction="sum")
    if kind == "l2":
        return ((mL[:, :K] - v / sizes) ** 2).sum()
    C = (mL - mL.mean(dim=0, keepdim=True)).t() @ (v - v.mean(dim=0, keepdim=True)) / mL.shape[0]
    off = ~torch.eye(mu.shape[1], K, dtype=torch.bool, device=mu.device)
    return (C[off] ** 2).sum()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "semi_time.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: there is nothing to time without it"
    lines = []

    def emit(what, t, **more):
        lines.append(json.dumps(dict({"what": what, "reps": args.reps, "median_ms": t[0], "spread_ms": t[1]}, **more)))
        print(lines[-1], flush=True)

    gen = torch.Generator(device="cuda").manual_seed(1)
    cpu = torch.Generator().manual_seed(2)
    st = _stream()
    D, K = 10, len(FACTORS)
    tab = _semilib.factor_table(DSPRITES, FACTORS)
    ps, pt = ctypes.addressof(tab[0]), ctypes.addressof(tab[1])
    sizes = torch.tensor(list(tab[0]), dtype=torch.float32, device="cuda")
    strides = torch.tensor(list(tab[1]), dtype=torch.int64, device="cuda")
    w = torch.ones(1, device="cuda")
    # ---- (a) the two launches alone
    for n in (64, 256, 1024, 2048):
        mu = torch.randn(n, D, generator=gen, device="cuda")
        rows = torch.randint(0, 737280, (n,), generator=cpu)
        rows[:n // 2] = -1
        rows = rows.to("cuda")
        idx = torch.nonzero(rows >= 0).view(-1)
        v = ((rows[idx].view(-1, 1) // strides) % sizes.long()).float()
        ws = torch.empty(_semilib.ws_doubles(n, D, K), dtype=torch.float64, device="cuda")
        out = torch.empty(_semilib.out_doubles(D, K), dtype=torch.float64, device="cuda")
        dmu = torch.empty_like(mu)
        tmu = mu.clone().requires_grad_(True)
        for kind in ("xent", "l2", "cov"):
            k = _semilib.KINDS[kind]

            def native(k=k):
                _semilib.call("dvae_semi_partials", mu.data_ptr(), 0, rows.data_ptr(), n, D, K, ps, pt, k, ws.data_ptr(), st)
                _semilib.call("dvae_semi_grad", mu.data_ptr(), 0, rows.data_ptr(), n, D, K, ps, pt, k, 0, w.data_ptr(), ws.data_ptr(),
                              dmu.data_ptr(), out.data_ptr(), None, st)

            def autograd(kind=kind):
                return torch.autograd.grad(torch_regulariser(tmu, idx, v, sizes, kind), [tmu])
            native()
            (g,) = autograd()
            err = float((g - dmu).abs().max() / g.abs().max())
            assert err < 1e-4, (kind, n, err)
            t = interleaved_ms({"native": native, "torch": autograd}, args.reps, inner=20)
            emit("dvae_semi_partials + dvae_semi_grad (value, dmu)", t["native"], sup_loss=kind, rows=n, D=D, K=K, grad_vs_torch_rel=err)
            emit("torch autograd, forward + backward of the same regulariser", t["torch"], sup_loss=kind, rows=n, D=D, K=K)
    # ---- (b) the whole step
    for img, B in (((3, 64, 64), 1024), ((1, 32, 32), 64)):
        steps = {}
        rows = torch.randint(0, 737280, (B,), generator=cpu)
        rows[:B // 2] = -1
        rows = rows.to("cuda")
        for name in ("betaH", "xent", "l2", "cov"):
            torch.manual_seed(3)
            model = init_specific_model("Burgess", img, 10).to("cuda")
            model.train()
            opt = torch.optim.Adam(model.parameters(), lr=5e-4)
            data = torch.rand((B,) + img, generator=gen, device="cuda")
            if name == "betaH":
                loss_f = get_loss_f("betaH", device=torch.device("cuda"), **HP)
                steps[name] = (lambda loss_f=loss_f, model=model, opt=opt, data=data: loss_f.fused_step(data, model, opt, None))
            else:
                loss_f = get_loss_f("s2vae", device=torch.device("cuda"), sup_loss=name, **HP)
                steps[name] = (lambda loss_f=loss_f, model=model, opt=opt, data=data: loss_f.fused_step(data, model, opt, None, labels=rows))
        for fn in steps.values():                                     # past the warm-up of every replay mode
            for _ in range(6):
                fn()
        t = interleaved_ms(steps, args.reps, inner=10)
        for name in steps:
            emit("whole training step, shipped replay setting", t[name], loss="betaH" if name == "betaH" else "s2vae " + name,
                 img=list(img), B=B, extra_vs_betaH_ms=round(t[name][0] - t["betaH"][0], 5))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
