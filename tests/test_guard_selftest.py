"""The guard-band harness (tests/guard.py) can fail: a torch-CPU stand-in "entry point" that honours the contract
passes ``check``, and six stand-ins that are each off by one are reported, each under the number of the assertion it
breaks.  No GPU: this is what shows that tests/test_gpu_bounds.py would notice, instead of an experiment that breaks a
kernel on the device."""
import pytest
import torch

import guard

NB, N = 3, 37


def _peek(t, k):
    """element k of t counted from its first element, also outside the view (a kernel's pointer arithmetic); outside
    the whole allocation -- where a device read returns a neighbour's bytes -- it gives 0"""
    off = t.storage_offset() + k
    if 0 <= off < t.untyped_storage().nbytes() // t.element_size():
        return torch.as_strided(t, (1,), (1,), off)[0]
    return torch.zeros((), dtype=t.dtype)


def _poke(t, k, value):
    off = t.storage_offset() + k
    if 0 <= off < t.untyped_storage().nbytes() // t.element_size():
        torch.as_strided(t, (1,), (1,), off)[0] = value


def stand_in(n, n_valid, bug=None):
    """y[b][i] = f[i-1] + f[i] + f[i+1] over the frame f = x[b*stride : b*stride + n_valid] padded with zeros to n
    (samples at or beyond n_valid are taken as zero, nothing outside the frame is read), every y[b][0..n) written"""
    def run(args, strides):
        x, y, sx, sy = args["x"], args["y"], strides["x"], strides["y"]
        for b in range(NB):
            f = torch.zeros(n + 2, dtype=y.dtype)
            f[1:1 + n_valid] = x[b * sx:b * sx + n_valid].to(y.dtype)
            out = f[:-2] + f[1:-1] + f[2:]
            if bug == "reads one before the base" and b == 0:
                out[0] += _peek(x, -1).to(y.dtype)
            if bug == "reads one past a block into the gap":
                out[n - 1] += _peek(x, b * sx + n).to(y.dtype)
            if bug == "uses a sample at n_valid":
                out[n_valid - 1] += _peek(x, b * sx + n_valid).to(y.dtype)
            m = n - 1 if (bug == "leaves the last promised element unwritten" and b == NB - 1) else n
            y[b * sy:b * sy + m] = out[:m]
            if bug == "writes one past a block":
                _poke(y, b * sy + n, 1.0)
        if bug == "writes one before the base":
            _poke(y, -1, 1.0)
    return run


def _case(dtype, gap, n_valid=N):
    g = torch.Generator().manual_seed(5)
    if dtype == torch.int8:
        x, ydt = torch.randint(-128, 128, (NB, n_valid), generator=g, dtype=torch.int8), torch.float32
    elif dtype.is_complex:
        x, ydt = torch.randn(NB, n_valid, generator=g, dtype=torch.float64).to(dtype) * (1 + 2j), dtype
    else:
        x, ydt = torch.randn(NB, n_valid, generator=g, dtype=dtype), dtype
    inputs = {"x": guard.In(x, N + gap, N, guard.TAIL + N - n_valid)}
    outputs = {"y": guard.Out(NB, N, ydt, N + gap + 2)}
    return inputs, outputs


@pytest.mark.parametrize("gap", [1, 4099])
@pytest.mark.parametrize("dtype", [torch.float32, torch.complex64, torch.float64, torch.complex128, torch.int8])
def test_a_correct_stand_in_passes(dtype, gap):
    for n_valid in (N, N - 9):
        inputs, outputs = _case(dtype, gap, n_valid)
        got = guard.check(stand_in(N, n_valid), inputs, outputs)
        assert torch.equal(got.tight["y"], got.guarded["y"]) and got.tight["y"].shape == (NB, N)
        f = torch.zeros(NB, N + 2, dtype=got.tight["y"].dtype)
        f[:, 1:1 + n_valid] = inputs["x"].blocks
        assert torch.equal(got.tight["y"], f[:, :-2] + f[:, 1:-1] + f[:, 2:])


def test_layout_and_poison():
    x = torch.arange(6, dtype=torch.float32).reshape(2, 3)
    v = guard.guarded_input(x, 5, lead=4, tail=2)
    assert v.storage_offset() == 4 and v.numel() == 5 + 3 + 2 and v.data_ptr() == v.untyped_storage().data_ptr() + 16
    whole = torch.as_strided(v, (4 + 8 + 2,), (1,), 0)
    assert torch.equal(torch.isnan(whole), torch.tensor([1, 1, 1, 1, 0, 0, 0, 1, 1, 0, 0, 0, 1, 1], dtype=torch.bool))
    c = guard.guarded_input(x.to(torch.complex128), 4, lead=1, tail=1)
    assert torch.isnan(c[3].real) and torch.isnan(c[3].imag) and c[4] == 3
    for fill, value in (("zero", 0), ("max", 32767)):
        r = guard.guarded_input(x.to(torch.int16), 4, lead=1, tail=1, fill=fill)
        assert r[3] == value and r[7] == value and r[4] == 3
    assert guard.LEAD % 2 == 1 and guard.LEAD > 4096 and guard.TAIL > 4096
    o = guard.guarded_output(2, 3, 5, torch.complex64, "cpu", lead=4, tail=2)
    o.view[5] = 1 + 1j                 # block 1, element 0
    o.view[4] = 2.0                    # in the gap
    outside, unwritten, payload = o.report()
    assert outside.tolist() == [4 + 4] and payload[1, 0] == 1 + 1j
    assert unwritten.tolist() == [[True, True, True], [False, True, True]]
    assert torch.isnan(payload[0, 0].real) and o.payload_bits()[0, 0].tolist() == [0x7FC0BEEF] * 2


BUGS = [("reads one before the base", "(2)", "(4)", N),
        ("reads one past a block into the gap", "(2)", "(4)", N),
        ("uses a sample at n_valid", "(2)", "(4)", N - 9),
        ("writes one past a block", "(3)", "(3)", N),
        ("writes one before the base", "(3)", "(3)", N),
        ("leaves the last promised element unwritten", "(1)", "(1)", N)]


@pytest.mark.parametrize("gap", [1, 4099])
@pytest.mark.parametrize("bug,kind_float,kind_int,n_valid", BUGS, ids=[b[0].replace(" ", "_") for b in BUGS])
def test_each_off_by_one_stand_in_is_reported(bug, kind_float, kind_int, n_valid, gap):
    """floating inputs: a poisoned read makes the result NaN (2); integer inputs cannot hold NaN: the two fills (0 and
    the type's maximum) then differ from each other and from the tight call (4)"""
    for dtype, kind in ((torch.complex64, kind_float), (torch.float64, kind_float), (torch.int8, kind_int)):
        inputs, outputs = _case(dtype, gap, n_valid)
        with pytest.raises(AssertionError) as e:
            guard.check(stand_in(N, n_valid, bug), inputs, outputs)
        msg = str(e.value)
        assert kind in msg, msg
        others = {"(1)", "(2)", "(3)", "(4)"} - {kind} - ({"(4)"} if kind == "(2)" else set())
        assert not any(k in msg for k in others), msg          # ... and nothing else is blamed (a NaN also differs)


def test_a_bar_replaces_bit_identity_only_when_asked():
    """an entry point shown not to be deterministic falls back to its parity bar for (4); the others stay"""
    flip = [0.0]

    def noisy(args, strides):
        stand_in(N, N)(args, strides)
        flip[0] += 1e-7
        args["y"][0] += flip[0]
    inputs, outputs = _case(torch.float32, 1)
    with pytest.raises(AssertionError, match=r"\(4\)"):
        guard.check(noisy, inputs, outputs)
    guard.check(noisy, inputs, outputs, bar=2e-5)
    with pytest.raises(AssertionError, match=r"\(3\)"):
        guard.check(stand_in(N, N, "writes one past a block"), inputs, outputs, bar=2e-5)
