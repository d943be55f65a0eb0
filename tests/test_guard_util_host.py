"""-m "not gpu": the guard-band harness (tests/guard_util.py) catches what it claims to, shown with small Python "kernels" on
CPU tensors -- every fake fault makes run_contract raise with the right argument and side named, a correct kernel passes --
and every entry point of the C-ABI has a memory-contract spec (tests/test_gpu_memory_contract.py) or a stated reason not to."""
import re

import pytest
import torch

import guard_util as G
from guard_util import run_contract, GuardError


def _build(n=37, dtype=torch.float32, ws=False):
    def build(al):
        x = al.inp("x", torch.arange(n, dtype=torch.float32) * 0.5 + 1.0)
        y = al.out("y", (n,), dtype=dtype, align=1 if dtype == torch.uint8 else 16)
        args = [x, y, n]
        if ws:
            args.append(al.ws("ws", (8,)))
        return args
    return build


def _poke(g, elem, value):
    """Store `value` at element offset `elem` relative to the payload, wherever that lands inside the argument's own allocation (a
    plain exact-size tensor has nothing around it that the test owns: the store is dropped, as it would hit a stranger's block)."""
    lo = g.start + elem * g.item
    if 0 <= lo and lo + g.item <= g.base.numel():
        g.base[lo:lo + g.item].view(g.dtype)[0] = value


def _peek(g, elem, stranger=3.25):
    lo = g.start + elem * g.item
    if 0 <= lo and lo + g.item <= g.base.numel():
        return g.base[lo:lo + g.item].view(g.dtype)[0].clone()
    return torch.tensor(stranger, dtype=g.dtype)        # a plain tensor's neighbour: some finite float of an earlier test


def k_ok(args):
    x, y, n = args[:3]
    y.t.copy_((x.t * 2).to(y.dtype))


def k_write_past(args):
    k_ok(args)
    _poke(args[1], args[2], 1.0)


def k_write_before(args):
    k_ok(args)
    _poke(args[1], -1, 1.0)


def k_skip_last(args):
    x, y, n = args[:3]
    y.t[:n - 1] = (x.t[:n - 1] * 2).to(y.dtype)


def k_clobber_input(args):
    k_ok(args)
    args[0].t[5] = -4.0


def k_reads_behind_input(args):
    x, y, n = args[:3]
    k_ok(args)
    y.t[n - 1] += _peek(x, n)


def k_reads_unwritten_ws(args):
    x, y, n, ws = args
    ws.t[:4] = 1.0                       # slots 4..7 are never written ...
    y.t.copy_(x.t * 2)
    y.t[0] += ws.t[6]                    # ... and one of them is added in


def _raises(fn, build, arg, sides, offset=None, count=None):
    with pytest.raises(GuardError) as ei:
        run_contract("fake", build, fn=fn, device="cpu")
    e = ei.value
    assert e.arg == arg, str(e)
    assert e.side in sides, str(e)
    if offset is not None:
        assert e.offset == offset, str(e)
    if count is not None:
        assert e.count == count, str(e)
    for word in (arg, e.side, "%+d" % e.offset, "%d element" % e.count):        # the report names all four
        assert word in str(e), str(e)
    return e


def test_a_correct_kernel_passes():
    runs = run_contract("fake", _build(), fn=k_ok, device="cpu")
    assert [r.variant for r in runs] == ["plain", "A", "B"]
    run_contract("fake", _build(dtype=torch.uint8), fn=k_ok, device="cpu")
    run_contract("fake", _build(ws=True), fn=lambda a: (a[3].t.fill_(1.0), k_ok(a)), device="cpu")


def test_write_one_element_past_the_payload():
    _raises(k_write_past, _build(37), "y", ("back guard",), offset=37, count=1)


def test_write_one_element_before_the_payload():
    _raises(k_write_before, _build(37), "y", ("front guard",), offset=-1, count=1)


def test_last_payload_element_left_unwritten():
    _raises(k_skip_last, _build(37), "y", ("unwritten payload",), offset=36, count=1)


def test_unwritten_element_under_a_mask_is_allowed_only_there():
    def build(al):
        x = al.inp("x", torch.arange(37, dtype=torch.float32))
        mask = torch.ones(37, dtype=torch.bool)
        mask[36] = False
        return [x, al.out("y", (37,), written=mask), 37]
    run_contract("fake", build, fn=k_skip_last, device="cpu")

    def skip_two(args):
        k_skip_last(args)
        args[1].t[3] = args[1].t[36]          # put the poison back at an element the mask does cover
    _raises(skip_two, build, "y", ("unwritten payload",), offset=3, count=1)


def test_modified_input():
    _raises(k_clobber_input, _build(37), "x", ("input modified",), offset=5, count=1)


def test_output_depends_on_the_first_guard_element_behind_an_input():
    _raises(k_reads_behind_input, _build(37), "y", ("differing bits", "non-finite output"), offset=36, count=1)


def test_read_of_an_unwritten_workspace_slot():
    _raises(k_reads_unwritten_ws, _build(37, ws=True), "y", ("differing bits", "non-finite output"), offset=0, count=1)


def test_single_byte_past_a_uint8_output():
    e = _raises(k_write_past, _build(37, dtype=torch.uint8), "y", ("back guard",), offset=37, count=1)
    assert e.variant == "A"
    # ... and an unwritten BYTE is found although a legitimate pixel may equal one run's poison byte
    _raises(k_skip_last, _build(37, dtype=torch.uint8), "y", ("unwritten payload",), offset=36, count=1)

    def k_poison_valued(args):                 # every result byte equals run A's poison byte: legitimate, not "unwritten"
        args[1].t.fill_(0x5A)
    run_contract("fake", _build(37, dtype=torch.uint8), fn=k_poison_valued, device="cpu")


def test_write_into_an_inputs_guard_and_a_workspaces_guard():
    def k(args):
        k_ok(args)
        _poke(args[0], 37 + 100, 0.0)
    _raises(k, _build(37), "x", ("back guard",), offset=137, count=1)

    def k2(args):
        args[3].t.fill_(0.0)
        k_ok(args)
        _poke(args[3], -3, 0.0)
        _poke(args[3], -2, 0.0)
    _raises(k2, _build(37, ws=True), "ws", ("front guard",), offset=-3, count=2)


def test_inout_argument_that_depends_on_stray_memory():
    def build(al):
        return [al.inout("p", torch.ones(9)), al.inp("g", torch.full((9,), 0.5))]

    def good(args):
        args[0].t.sub_(args[1].t)

    def bad(args):
        good(args)
        args[0].t[8] += _peek(args[1], 9)
    run_contract("fake", build, fn=good, device="cpu")
    _raises(bad, build, "p", ("differing bits", "non-finite output"), offset=8, count=1)


@pytest.mark.parametrize("shape,dtype,want", [((7,), torch.float32, 64 << 10), ((5, 3, 64, 64), torch.float32, 32 * 3 * 64 * 64 * 4),
                                              ((2, 512), torch.float32, 64 << 10), ((1 << 20, 3), torch.uint8, 64 << 10),
                                              ((2, 1 << 20), torch.float32, 64 << 20), ((4, 1024), torch.int64, 32 * 8192)])
def test_guard_size_condition(shape, dtype, want):
    assert G.guard_bytes(shape, dtype) == want


@pytest.mark.parametrize("dtype,align", [(torch.float32, 16), (torch.float32, 4), (torch.uint8, 4), (torch.uint8, 1),
                                         (torch.int64, 16), (torch.int32, 16), (torch.float32, 256)])
def test_alignment_guards_and_poison_of_both_variants(dtype, align):
    for variant in ("A", "B"):
        g = G.Guarded((3, 50), dtype, G.OUT, variant, align=align, name="t")
        assert g.t.data_ptr() == g.ptr and g.t.is_contiguous() and g.t.shape == (3, 50)
        if variant == "A" or align == 256:
            assert g.ptr % 256 == 0
        else:
            assert g.ptr % align == 0 and g.ptr % (2 * align) != 0
        assert g.start >= G.guard_bytes((3, 50), dtype) and g.base.numel() - g.end >= G.guard_bytes((3, 50), dtype)
        assert bool(g.poisoned().all())
        if dtype == torch.float32:
            assert bool(torch.isnan(g.t).all())                       # outputs: NaN in both variants ...
            bits = g.t.view(torch.int32)
            assert int(bits.min()) == int(bits.max())
            w = G.Guarded((4,), dtype, G.WS, variant, name="w")
            assert bool(torch.isnan(w.t).all()) == (variant == "A")   # ... workspaces: NaN in A, large and finite in B
            if variant == "B":
                assert float(w.t[0]) == pytest.approx(-1e30, rel=1e-6)
        with pytest.raises(GuardError, match="unwritten payload"):
            g.check_after()
        g.t.zero_()
        g.check_after()
    a = G.Guarded((4,), dtype, G.OUT, "A", align=align)
    b = G.Guarded((4,), dtype, G.OUT, "B", align=align)
    assert not torch.equal(a.payload_bits(), b.payload_bits())         # the two poisons differ in every byte position
    assert bool((a.payload_bits() != b.payload_bits()).all())


def test_input_roundtrip_and_plain_variant():
    data = torch.randn(5, 6)
    for variant in ("plain", "A", "B"):
        g = G.Guarded(data.shape, torch.float32, G.IN, variant, data=data, name="x")
        assert torch.equal(g.t, data)
        g.check_after()
    with pytest.raises(ValueError):
        G.Guarded((3,), torch.float32, G.IN, "A")
    with pytest.raises(ValueError):
        G.Guarded((3,), torch.float32, G.OUT, "A", data=torch.zeros(3))


# ---- every entry point has a spec ------------------------------------------------------------------------------------------
# Entry points the memory contract does not apply to, each with its reason.  Only these kinds may be listed: the version /
# error queries, host-only size / shape / capability queries, stream and event primitives, the plan runner and the collectives.
NO_CONTRACT = {
    "dvae_version": "host only: returns a constant",
    "dvae_last_error": "host only: returns the thread's error text",
    "dvae_conv_wgrad_ws_floats": "host-only size query",
    "dvae_latent_entropy_ws_floats": "host-only size query",
    "dvae_recon_rows_ws_floats": "host-only size query (writes one host long)",
    "dvae_image_grid_shape": "host-only shape query (writes two host longs)",
    "dvae_fc_chain_rows": "host-only schedule query",
    "dvae_reparam_kl_blocks": "host-only block-count query",
    "dvae_u8_fused_supported": "host-only capability query",
    "dvae_plan_op": "host only: name -> op code",
    "dvae_plan_run": "replays recorded calls of the other entry points: no memory traffic of its own (the whole-step poison test runs it)",
    "dvae_stream_order": "stream primitive: touches no caller memory",
    "dvae_stream_create": "stream primitive: writes one host pointer",
    "dvae_event_record": "event primitive: touches no caller memory",
    "dvae_event_wait": "event primitive: touches no caller memory",
}
_ALLOWED = re.compile(r"^dvae_(version|last_error|\w+_ws_floats|image_grid_shape|fc_chain_rows|reparam_kl_blocks|u8_fused_supported|"
                      r"plan_op|plan_run|stream_\w+|event_\w+|comm_\w+)$")


def test_every_entry_point_has_a_memory_contract_spec_or_a_reason():
    from disvae_amd import _lib
    import test_gpu_memory_contract as M
    covered = {s.entry for s in M.SPECS}
    excluded = dict(NO_CONTRACT)
    excluded.update({n: "RCCL collective / communicator management: buffers are RCCL's to police (tests/test_gpu_ddp.py)"
                     for n in _lib.SIGNATURES if n.startswith("dvae_comm_")})
    for n, why in excluded.items():
        assert _ALLOWED.match(n), "%s may not be excluded from the memory contract" % n
        assert why and n in _lib.SIGNATURES, n
    assert not (covered & set(excluded)), sorted(covered & set(excluded))
    missing = sorted(set(_lib.SIGNATURES) - covered - set(excluded))
    assert not missing, "entry points without a memory-contract spec: %s" % missing
    assert not (covered - set(_lib.SIGNATURES)), sorted(covered - set(_lib.SIGNATURES))
    ids = [s.id for s in M.SPECS]
    assert len(ids) == len(set(ids))
