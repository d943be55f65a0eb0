"""CPU: tests/default_noise.py states the reference's draw order -- pinned to an independent statement of it.

oracle.disvae_oracle.OracleTrainer.train_iteration(data) draws its own noise from the CPU generator in the reference's order
(FactorVAE: the discarded full-batch draw of training.py:153, eps of losses.py:254, eps2 of :286, then the D permutations of
:505; every other loss: one [B, D] draw, vae.py:67).  A second OracleTrainer is fed what default_noise.predraw drew from the
equally seeded generator (on the CPU both of the helper's streams are that one generator).  Same arithmetic on the same
numbers: losses and parameters are bit-identical, or the helper -- which the GPU test (tests/test_gpu_default_noise.py)
feeds to the injected-noise step -- draws in another order than the reference.
"""
import pytest
import torch

from oracle import disvae_oracle as O
from default_noise import predraw, device_draws, cpu_draws, rng_states
from test_oracle_golden import HP

STEPS = 3


def test_shapes_per_iteration():
    assert device_draws("factor", 9, 10) == [(9, 10), (4, 10), (4, 10)] and cpu_draws("factor", 9, 10) == [4] * 10
    for loss in ("VAE", "betaH", "betaB", "btcvae"):
        assert device_draws(loss, 9, 10) == [(9, 10)] and cpu_draws(loss, 9, 10) == []


@pytest.mark.parametrize("loss,img,B", [("VAE", (1, 32, 32), 8), ("factor", (1, 64, 64), 9)])
def test_helper_order_is_the_oracle_trainers(loss, img, B):
    D, seed = 10, 77
    hp = dict(HP, n_data=737280)
    torch.manual_seed(5)                                   # initialisation consumes the CPU generator: before any seeding
    params = O.init_vae_params(img, D)
    dparams = O.init_disc_params(D) if loss == "factor" else None
    make = lambda: O.OracleTrainer(loss, hp, img, D, lr=5e-4, lr_disc=HP["lr_disc"], steps_anneal=HP["reg_anneal"],
                                   params=params, dparams=dparams)
    gen = torch.Generator().manual_seed(6)                 # data: a private generator
    batches = [torch.rand((B,) + img, generator=gen) for _ in range(STEPS)]

    noise, _, cpu_state = predraw(loss, [B] * STEPS, D, None, seed, "cpu")
    fed = make()
    if loss == "factor":
        assert all(n["eps1"].shape == (B // 2, D) and n["perms"].shape == (D, B // 2) for n in noise)
        fed_losses = [fed.train_iteration(x, eps=n["eps1"], eps2=n["eps2"], perms=list(n["perms"]))[0]
                      for x, n in zip(batches, noise)]
    else:
        fed_losses = [fed.train_iteration(x, eps=n["eps"])[0] for x, n in zip(batches, noise)]

    own = make()
    torch.manual_seed(seed)
    own_losses = [own.train_iteration(x)[0] for x in batches]
    assert torch.equal(rng_states("cpu")[1], cpu_state), "the helper consumed the generator differently"
    assert own_losses == fed_losses, (own_losses, fed_losses)
    for k in own.params:
        assert torch.equal(own.params[k], fed.params[k]), k
    if loss == "factor":
        for k in own.dparams:
            assert torch.equal(own.dparams[k], fed.dparams[k]), k
