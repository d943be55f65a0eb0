"""Cost of the DIP-VAE regulariser (libdvae_dip_hip.so, csrc/dip_cov.hip) and of the training step that carries it.

(a) The two launches alone (dvae_dip_moments + dvae_dip_grad, type II: value, dmu and dlv) at B = 64, 256, 1024, 2048 with D = 10
    and B = 1024 with D = 32, next to torch autograd -- forward + backward of the same regulariser written with torch ops -- on
    the same GPU.  The gradients of both are compared before timing.
(b) The whole dipI / dipII training step against the VAE step of the same build, (3, 64, 64) at B = 1024 and (1, 32, 32) at
    B = 64, the shipped replay setting: what the regulariser adds to a step, to be held against (a).

Device events around each call; the candidates are INTERLEAVED (one repeat of each in turn, `--reps` rounds after a warm-up), so a
drift of the clocks lands on all of them; the median and the spread [min, max] are reported.  Inputs from a seed.  Prints one JSON
line per measurement and writes them to --out.

    python tools/dip_time.py [--reps 30] [--out profiles/dip_time.jsonl]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "disentangling-vae_amd")]

import torch  # noqa: E402

from disvae_amd import _diplib  # noqa: E402
from disvae_amd.engine import _stream  # noqa: E402
from disvae_amd.models.losses import get_loss_f  # noqa: E402
from disvae_amd.models.vae import init_specific_model  # noqa: E402

LAMBDA_OD, LAMBDA_D = 10.0, 10.0
HP = dict(rec_dist="bernoulli", reg_anneal=10000, betaH_B=4, betaB_initC=0, betaB_finC=25, betaB_G=1000, factor_G=6.4,
          lr_disc=1e-4, btcvae_A=1, btcvae_B=6.4, btcvae_G=1, n_data=202599, latent_dim=10)


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


def torch_regulariser(mu, logvar):
    B = mu.shape[0]
    c = mu - mu.mean(dim=0, keepdim=True)
    C = c.t() @ c / B + torch.diag(logvar.exp().mean(dim=0))
    diag = C.diagonal()
    off = C - torch.diag(diag)
    return LAMBDA_OD * (off ** 2).sum() + LAMBDA_D * ((diag - 1.0) ** 2).sum()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dip_time.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: there is nothing to time without it"
    lines = []

    def emit(what, t, **more):
        lines.append(json.dumps(dict({"what": what, "reps": args.reps, "median_ms": t[0], "spread_ms": t[1]}, **more)))
        print(lines[-1], flush=True)

    gen = torch.Generator(device="cuda").manual_seed(1)
    st = _stream()
    # ---- (a) the two launches alone
    for B, D in ((64, 10), (256, 10), (1024, 10), (2048, 10), (1024, 32)):
        mu = torch.randn(B, D, generator=gen, device="cuda")
        lv = -3 * torch.rand(B, D, generator=gen, device="cuda")
        ws = torch.empty(_diplib.ws_doubles(B, D), dtype=torch.float64, device="cuda")
        out = torch.empty(_diplib.out_doubles(D), dtype=torch.float64, device="cuda")
        dmu, dlv = torch.empty_like(mu), torch.empty_like(mu)

        def native():
            _diplib.call("dvae_dip_moments", mu.data_ptr(), lv.data_ptr(), B, D, ws.data_ptr(), st)
            _diplib.call("dvae_dip_grad", mu.data_ptr(), lv.data_ptr(), B, D, LAMBDA_OD, LAMBDA_D, ws.data_ptr(), dmu.data_ptr(),
                         dlv.data_ptr(), out.data_ptr(), None, st)
        tmu, tlv = mu.clone().requires_grad_(True), lv.clone().requires_grad_(True)

        def autograd():
            return torch.autograd.grad(torch_regulariser(tmu, tlv), [tmu, tlv])
        native()
        gmu, glv = autograd()
        err = max(float((gmu - dmu).abs().max() / gmu.abs().max()), float((glv - dlv).abs().max() / glv.abs().max()))
        assert err < 1e-4, err
        t = interleaved_ms({"native": native, "torch": autograd}, args.reps, inner=20)
        emit("dvae_dip_moments + dvae_dip_grad (type II: value, dmu, dlv)", t["native"], B=B, D=D, grad_vs_torch_rel=err)
        emit("torch autograd, forward + backward of the same regulariser", t["torch"], B=B, D=D)
    # ---- (b) the whole step
    for img, B in (((3, 64, 64), 1024), ((1, 32, 32), 64)):
        steps = {}
        for loss in ("VAE", "dipI", "dipII"):
            torch.manual_seed(3)
            model = init_specific_model("Burgess", img, 10).to("cuda")
            model.train()
            opt = torch.optim.Adam(model.parameters(), lr=5e-4)
            loss_f = get_loss_f(loss, device=torch.device("cuda"), **HP)
            data = torch.rand((B,) + img, generator=gen, device="cuda")
            steps[loss] = (lambda loss_f=loss_f, model=model, opt=opt, data=data: loss_f.fused_step(data, model, opt, None))
        for fn in steps.values():                                     # past the warm-up of every replay mode
            for _ in range(6):
                fn()
        t = interleaved_ms(steps, args.reps, inner=10)
        for loss in steps:
            emit("whole training step, shipped replay setting", t[loss], loss=loss, img=list(img), B=B,
                 extra_vs_VAE_ms=round(t[loss][0] - t["VAE"][0], 5))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
