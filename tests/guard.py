"""Guard bands around the device arguments of an entry point (include/prcore.h, Conventions: an entry point reads a
block only inside [b*stride, b*stride + extent), writes only inside the documented output extents, needs only
element alignment, and no result depends on what a plan was used for before).

Every argument lives in ONE allocation laid out as

    lead | block 0 | gap | block 1 | gap | ... | block nb-1 | tail

and the entry point is handed the view that starts at block 0.  Inputs hold poison everywhere outside the payload (NaN
in every component for floating types; 0, then the type's maximum, for integer types -- the case runs once per fill).
Outputs hold a sentinel everywhere: a quiet NaN with a recognisable payload, compared as bits.  ``check`` runs the
entry point on the guarded arguments and on tight, freshly allocated, exactly-sized ones and asserts

    (1) every promised output element was written,
    (2) every written output element is finite,
    (3) every sentinel element outside the declared extents is bit-for-bit untouched,
    (4) the payload is bit-identical to the tight call's (and, for integer inputs, between the two fills).

An over-read shows as a NaN in a result (2) or as a difference from the tight call (4); an over-write as a changed
sentinel (3).  What it cannot see is an over-read whose value is loaded and then discarded.

Plain torch, any device: tests/test_guard_selftest.py runs it on the CPU against stand-ins that are off by one.
"""
from dataclasses import dataclass
from typing import Optional

import torch

LEAD = 4099        # odd: the base is element-aligned only; longer than one 4096-point piece, so a prefetch one piece
TAIL = 4099        # past the end still lands in owned memory

# the component type whose bits carry the sentinel, and the sentinel, per component size
_BITS = {1: (torch.uint8, 0xA5), 2: (torch.int16, 0x7E5A), 4: (torch.int32, 0x7FC0BEEF), 8: (torch.int64, 0x7FF80000DEADBEEF)}


def _components(dtype):
    """(component bit type, sentinel, components per element)"""
    comps = 2 if dtype.is_complex else 1
    bits, sentinel = _BITS[torch.empty(0, dtype=dtype).element_size() // comps]
    return bits, sentinel, comps


def _poison(dtype, fill):
    if dtype.is_complex:
        return complex(float("nan"), float("nan"))
    if dtype.is_floating_point:
        return float("nan")
    return 0 if fill == "zero" else torch.iinfo(dtype).max


def guarded_input(blocks, stride, lead=LEAD, tail=TAIL, fill="nan"):
    """``blocks``: [nblocks, extent] payload.  Returns the flat view that starts at block 0 (its data_ptr() honours the
    offset) of one allocation ``lead | block 0 | gap | ... | tail`` whose every non-payload element holds the poison:
    NaN in every component for floating types (whatever ``fill``), else 0 (fill="zero") or the type's maximum ("max")."""
    nb, extent = blocks.shape
    assert stride >= extent and nb >= 1
    span = (nb - 1) * stride + extent
    base = torch.empty(lead + span + tail, dtype=blocks.dtype, device=blocks.device)
    base.fill_(_poison(blocks.dtype, fill))
    base.as_strided((nb, extent), (stride, 1), lead).copy_(blocks)
    return base[lead:]


class GuardedOutput:
    """One allocation ``lead | block 0 | gap | ... | tail`` filled with the sentinel.  ``view`` is the flat typed view
    from block 0; ``report()`` says what happened to it."""

    def __init__(self, nblocks, extent, stride, dtype, device, lead=LEAD, tail=TAIL):
        assert stride >= extent and nblocks >= 1
        self.nblocks, self.extent, self.stride, self.lead = nblocks, extent, stride, lead
        self.bits_dtype, self.sentinel, self.comps = _components(dtype)
        self.total = lead + (nblocks - 1) * stride + extent + tail
        self._bits = torch.full((self.total * self.comps,), self.sentinel, dtype=self.bits_dtype, device=device)
        self._typed = self._bits.view(dtype)
        self.view = self._typed[lead:]

    def payload(self):
        """[nblocks, extent] typed view of the declared extents"""
        return self._typed.as_strided((self.nblocks, self.extent), (self.stride, 1), self.lead)

    def payload_bits(self):
        """the same as component bits [nblocks, extent, comps]: what 'bit-identical' compares"""
        return self._bits.as_strided((self.nblocks, self.extent, self.comps),
                                     (self.stride * self.comps, self.comps, 1), self.lead * self.comps)

    def report(self):
        """(outside, unwritten, payload): allocation-relative element indices outside the declared extents whose
        sentinel changed (block 0 starts at ``lead``); bool [nblocks, extent], True where an element inside them still
        holds the sentinel in every component; the payload view"""
        changed = (self._bits != self.sentinel).view(self.total, self.comps).any(dim=1)
        inside = torch.zeros(self.total, dtype=torch.bool, device=changed.device)
        inside.as_strided((self.nblocks, self.extent), (self.stride, 1), self.lead).fill_(True)
        outside = torch.nonzero(changed & ~inside).flatten()
        unwritten = ~changed.as_strided((self.nblocks, self.extent), (self.stride, 1), self.lead)
        return outside, unwritten, self.payload()


def guarded_output(nblocks, extent, stride, dtype, device, lead=LEAD, tail=TAIL):
    return GuardedOutput(nblocks, extent, stride, dtype, device, lead, tail)


@dataclass
class In:
    """a device input: ``blocks`` [nblocks, extent] payload, read at ``stride`` (None: the extent, i.e. one block or a
    dense batch -- lead and tail only).  The tight call reads the same payload at ``tight_stride`` (None: the extent)
    with zeros between the blocks.  ``tail``: extra owned elements after the last block, for an entry point whose
    documented extent is longer than the payload (a CAF frame with n_valid < n)."""
    blocks: torch.Tensor
    stride: Optional[int] = None
    tight_stride: Optional[int] = None
    tail: int = TAIL


@dataclass
class Out:
    """a device output of ``nblocks`` blocks of ``extent`` elements written at ``stride`` (None: dense).  ``promised``:
    None = the header promises every element of the extents is written; else bool [nblocks, extent] of the promised
    ones (the rest may stay untouched).  ``finite`` = False for outputs that are not numbers (packed records)."""
    nblocks: int
    extent: int
    dtype: torch.dtype
    stride: Optional[int] = None
    tight_stride: Optional[int] = None
    promised: Optional[torch.Tensor] = None
    finite: bool = True


@dataclass
class Checked:
    tight: dict        # name -> [nblocks, extent] payload of the tight call
    guarded: dict      # name -> the same of the (last) guarded call


def _first(idx, n=8):
    return idx[:n].tolist()


def check(run, inputs, outputs, bar=None):
    """``run(args, strides)`` calls the entry point once: ``args[name]`` is the tensor to pass for that argument (block 0
    first), ``strides[name]`` its stride in elements; it returns after the work is complete.  ``inputs`` / ``outputs``:
    name -> In / Out.  Asserts (1)-(4) of the module docstring; the message of a failure names each one that broke.
    ``bar``: None = (4) is bit identity; a number = for an entry point shown not to be deterministic, (4) is
    max|a-b| / max|b| < bar.  Returns the payloads, so the caller can hold the tight call to its oracle."""
    fills = ("nan",)
    if any(not (i.blocks.dtype.is_floating_point or i.blocks.dtype.is_complex) for i in inputs.values()):
        fills = ("zero", "max")
    device = next(iter(inputs.values())).blocks.device
    broke = []

    def launch(guarded, fill):
        args, strides, outs = {}, {}, {}
        for name, i in inputs.items():
            extent = i.blocks.shape[1]
            if guarded:
                strides[name] = extent if i.stride is None else i.stride
                args[name] = guarded_input(i.blocks, strides[name], LEAD, i.tail, fill)
            else:
                strides[name] = extent if i.tight_stride is None else i.tight_stride
                flat = torch.zeros((i.blocks.shape[0] - 1) * strides[name] + extent, dtype=i.blocks.dtype, device=device)
                flat.as_strided(i.blocks.shape, (strides[name], 1), 0).copy_(i.blocks)
                args[name] = flat
        for name, o in outputs.items():
            if guarded:
                strides[name] = o.extent if o.stride is None else o.stride
                outs[name] = GuardedOutput(o.nblocks, o.extent, strides[name], o.dtype, device)
            else:
                strides[name] = o.extent if o.tight_stride is None else o.tight_stride
                outs[name] = GuardedOutput(o.nblocks, o.extent, strides[name], o.dtype, device, 0, 0)
            args[name] = outs[name].view
        run(args, strides)
        return outs

    tight = launch(False, None)
    runs = {fill: launch(True, fill) for fill in fills}
    for fill, outs in runs.items():
        tag = "" if fill == "nan" else f" [gaps filled with {fill}]"
        for name, o in outputs.items():
            outside, unwritten, payload = outs[name].report()
            if outside.numel():
                rel = [int(k) - outs[name].lead for k in _first(outside)]
                broke.append(f"(3) {name}{tag}: {outside.numel()} sentinel element(s) outside the declared extents "
                             f"were overwritten, at offsets {rel} from block 0 (stride {outs[name].stride}, "
                             f"extent {o.extent})")
            must = ~unwritten.new_zeros(unwritten.shape) if o.promised is None else o.promised.to(unwritten.device)
            missing = torch.nonzero(unwritten & must)
            if missing.numel():
                broke.append(f"(1) {name}{tag}: {missing.shape[0]} promised element(s) were not written, first "
                             f"(block, index) {_first(missing, 4)}")
            if o.finite and (o.dtype.is_floating_point or o.dtype.is_complex):
                bad = torch.nonzero(~unwritten & ~torch.isfinite(payload))
                if bad.numel():
                    broke.append(f"(2) {name}{tag}: {bad.shape[0]} written element(s) are not finite, first "
                                 f"(block, index) {_first(bad, 4)}")
            for other, other_what in ((tight[name], "the tight call"), (runs[fills[0]][name], f"the {fills[0]} fill")):
                if other is outs[name]:
                    continue
                if bar is None:
                    diff = torch.nonzero((outs[name].payload_bits() != other.payload_bits()).any(dim=2))
                    if diff.numel():
                        broke.append(f"(4) {name}{tag}: {diff.shape[0]} payload element(s) differ in bits from "
                                     f"{other_what}, first (block, index) {_first(diff, 4)}")
                else:
                    a, b = payload.to(torch.complex128), other.payload().to(torch.complex128)
                    err = float((a - b).abs().max() / b.abs().max())
                    if not err < bar:
                        broke.append(f"(4) {name}{tag}: payload differs from {other_what} by {err:.3g} "
                                     f"(peak-normalised), bar {bar:g}")
    assert not broke, "guard check failed:\n  " + "\n  ".join(broke)
    last = runs[fills[-1]]
    return Checked({k: v.payload() for k, v in tight.items()}, {k: v.payload() for k, v in last.items()})
