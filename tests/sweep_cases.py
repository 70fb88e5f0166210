"""Seeded random-shape sweep of the entry points added after kind 25 of tests/fuzz_parity.py: case generators and runners.

One *kind* per entry-point family of include/prcore.h (the section of the header against its kind):

    LS_Filter_SVD -> ls_svd | ECA_Filter -> eca | GAL_JPE -> gal | order-statistic CFAR -> cfar_os | target tracking -> track |
    plot extraction -> plots | track-before-detect -> tbd | single-target tracker -> strack | persistence -> persistence |
    display frames -> display | Welch spectra -> welch | FIR decimator and the rest of signal_utils.py -> preproc |
    exact cross-ambiguity patches -> patch | joint least-squares removal of strong echoes -> echo

A kind has ``draw(rng) -> case`` (a dict of plain sizes, options and one input seed: repr(case) reproduces it),
``expected(case)`` (from the oracle the kind's own GPU test uses, computed once per case and shared), ``run(case, ...)`` (the
shipped Python entry point on the GPU) and ``check(case, f, got, want)`` at the bars of that GPU test.  Shapes are drawn
around the points where a kernel switches form: the named constants beside each kind, with their source, and the STRADDLE
table that tests/test_sweep_host.py holds the seeded lists to.

Results have one shape for every kind: ``{"frames": [per frame / block / stream / channel, a tuple of arrays], "whole": what
belongs to the call as a whole, or None}``.  ``run(case, order=[...])`` runs the listed frames only, in that order: a batched
kind promises that a frame's bytes do not depend on its position or its neighbours.  ``fill`` is the byte a caller-owned
workspace (and every output buffer the runner allocates itself) holds before the call.  ``plain=True`` leaves the
process-wide switches alone (the four-thread test).

No GPU is needed to import this module, to draw or to compute ``expected``."""
import math
import zlib

import numpy as np

SEED = 3               # a seed whose 24-case lists cross every switch point of STRADDLE (tests/test_sweep_host.py holds them to it)
NCASES = 24            # per kind
THREAD_CASES = 6       # per kind and thread in the four-thread test

_EXPECTED = {}
_INPUTS = {}


def pick(rng, seq):
    return seq[int(rng.integers(len(seq)))]


def seeded(case, salt=0):
    return np.random.default_rng([int(case["seed"]), salt])


def cwhite(rng, shape):
    return ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * math.sqrt(0.5)).astype(np.complex64)


def dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dev_bytes(nbytes, fill):
    """a caller-owned device buffer of ``nbytes`` holding ``fill`` in every byte (None: whatever the allocator returns)"""
    import torch
    if fill is None:
        return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device="cuda")
    return torch.full((max(int(nbytes), 1),), int(fill), dtype=torch.uint8, device="cuda")


def dev_out(shape, dtype, fill):
    """an output tensor whose bytes hold ``fill`` before the call"""
    import torch
    n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
    if not n:
        return torch.empty(shape, dtype=dtype, device="cuda")
    return dev_bytes(n, 0xA5 if fill is None else fill)[:n].view(dtype).view(*shape)


def untouched(gap, fill):
    """whether the elements between two blocks of an output from ``dev_out`` still hold what they held before the call"""
    return np.bool_((np.ascontiguousarray(gap).view(np.uint8) == (0xA5 if fill is None else fill)).all())


def to_bytes(obj):
    """the bytes of a result (nested tuples / lists / dicts of arrays and scalars): what 'bit-identical' compares"""
    if obj is None:
        return b"N"
    if isinstance(obj, dict):
        return b"".join(k.encode() + to_bytes(obj[k]) for k in sorted(obj))
    if isinstance(obj, (tuple, list)):
        return b"(" + b"".join(to_bytes(v) + b"," for v in obj) + b")"
    a = np.ascontiguousarray(obj)
    return str(a.dtype).encode() + str(a.shape).encode() + a.tobytes()


def cases(kind, seed=SEED, n=NCASES):
    """the seeded case list of one kind; it does not depend on any other kind having been drawn"""
    rng = np.random.default_rng([int(seed), zlib.crc32(kind.encode())])
    return [KINDS[kind].draw(rng) for _ in range(n)]


def expected(case):
    key = repr(case)
    if key not in _EXPECTED:
        _EXPECTED[key] = KINDS[case["kind"]].expected(case)
    return _EXPECTED[key]


def inputs(case):
    key = repr(case)
    if key not in _INPUTS:
        if len(_INPUTS) > 400:
            _INPUTS.clear()
        _INPUTS[key] = KINDS[case["kind"]].inputs(case)
    return _INPUTS[key]


def run(case, order=None, fill=None, plain=False):
    return KINDS[case["kind"]].run(case, order, fill, plain)


def check(case, got, order=None):
    """a result of ``run`` against ``expected`` at the kind's bars; an AssertionError names the case"""
    kind, want = KINDS[case["kind"]], expected(case)
    order = list(range(kind.nframes(case))) if order is None else order
    try:
        assert len(got["frames"]) == len(order)
        for pos, f in enumerate(order):
            kind.check(case, f, got["frames"][pos], want)
        if got["whole"] is not None:
            kind.check_whole(case, got["whole"], want)
    except AssertionError as e:
        raise AssertionError(f"{case!r}: {e}") from e


class Kind:
    name = header = ""     # header: how the kind's section of include/prcore.h begins
    STRADDLE = {}          # name -> (case -> a value or a set of values, the values the seeded list must hold)

    @staticmethod
    def nframes(case):
        return 1

    @classmethod
    def orders(cls, case):
        """the frame lists of the position pass: every frame alone, and the stack reversed (other position, other neighbours)"""
        n = cls.nframes(case)
        return [[f] for f in range(n)] + ([list(range(n))[::-1]] if n > 1 else [])

    @staticmethod
    def conditioned(case, want):
        """raises AssertionError where the oracle alone is not to be trusted on this case (host test: never)"""

    @staticmethod
    def check_whole(case, got, want):
        raise AssertionError("this kind has no whole-call result")

    @staticmethod
    def extra_passes(case, base):
        """[(label, frames)] of further runs whose frames must equal ``base``'s bit for bit (e.g. the other storage path)"""
        return []


# ---- cfar_os ---------------------------------------------------------------------------------------------------------------------
class CfarOs(Kind):
    name, header = "cfar_os", "order-statistic CFAR"
    TILE_ROWS, TILE_COLS = 16, 64          # CO_TY, CO_TX of csrc/cfar_os.hip: the outputs of one workgroup
    AMPS = (1.0, 30.0, 0.01)

    @staticmethod
    def draw(rng):
        fw = pick(rng, [3, 4, 9, 10, 17, 18, 33])
        wide = fw >= 33                     # the oracle sorts fw^2 planes per frame: the widest window stays on small frames
        H = pick(rng, [5, 15, 16, 17] if wide else [3, 5, 15, 16, 17, 31, 33, 40])
        W = pick(rng, [7, 63, 64, 65] if wide else [5, 7, 63, 64, 65, 129, 150])
        dtype = pick(rng, ["f32", "f32", "c64"])
        return dict(kind="cfar_os", H=H, W=W, fw=fw, gw=min(pick(rng, [0, 1, 2, 4, 6]), fw - 2),
                    rank=pick(rng, ["one", "nt", "default", "mid"]), scale=pick(rng, ["reference", "plain"]), dtype=dtype,
                    values="gauss" if dtype == "c64" else pick(rng, ["rayleigh", "rayleigh", "quantised", "signed"]),
                    noise=bool(rng.integers(2)), thresh=bool(rng.integers(2)), nframes=int(rng.integers(1, 4)),
                    seed=int(rng.integers(1 << 30)))

    @staticmethod
    def nframes(case):
        return case["nframes"]

    @staticmethod
    def rank_of(case):
        import cfar_os_oracle as OS
        nt = OS.training_cells(case["fw"], case["gw"])
        return {"one": 1, "nt": nt, "default": None, "mid": math.ceil(nt / 2)}[case["rank"]]

    @staticmethod
    def inputs(case):
        out = []
        for f in range(case["nframes"]):
            rng, shape, amp = seeded(case, f), (case["H"], case["W"]), np.float32(CfarOs.AMPS[f])
            if case["values"] == "gauss":
                out.append(cwhite(rng, shape) * amp)
            elif case["values"] == "rayleigh":
                out.append(np.abs(cwhite(rng, shape)).astype(np.float32) * amp)
            elif case["values"] == "quantised":
                out.append(rng.integers(0, 4, shape).astype(np.float32))
            else:
                x = rng.standard_normal(shape).astype(np.float32) * amp
                x.flat[0], x.flat[-1] = -0.0, 0.0
                out.append(x)
        return out

    @staticmethod
    def expected(case):
        import cfar_os_oracle as OS
        frames = []
        for x in inputs(case):
            mag = np.abs(x) if case["dtype"] == "c64" else x
            z = OS.noise(mag, case["fw"], case["gw"], CfarOs.rank_of(case))
            frames.append(dict(mag=mag, z=z, ratio=OS.ratios(mag, z, case["scale"])))
        r0 = frames[0]["ratio"]
        fin = r0[np.isfinite(r0)]
        return dict(frames=frames, thr=float(np.percentile(fin, 90)) if fin.size else 1.0)

    @staticmethod
    def run(case, order, fill, plain):
        from passiveradar_amd.target_detection import CFAR_2D_OS
        xs = inputs(case)
        order = list(range(case["nframes"])) if order is None else order
        X = np.stack([xs[f] for f in order])
        fw, gw, k, scale = case["fw"], case["gw"], CfarOs.rank_of(case), case["scale"]
        thr = expected(case)["thr"] if case["thresh"] else None
        if fill is None:
            r = CFAR_2D_OS(X, fw, gw, rank=k, scale=scale, return_noise=case["noise"])
            ratio, z = r if case["noise"] else (r, None)
            hit = CFAR_2D_OS(X, fw, gw, thr, rank=k, scale=scale) if case["thresh"] else None
        else:                               # the same call on caller-owned buffers: workspace and outputs hold ``fill``
            import torch
            from passiveradar_amd import _lib, engine
            xd, N = dev(X), X.shape[0]

            def call(t):
                d = engine.cfar_os_desc(case["H"], case["W"], fw, gw, k, scale, case["dtype"] == "c64", t)
                ws = dev_bytes(engine.cfar_os_workspace_bytes(d, N), fill)
                o = dev_out(X.shape, torch.float32, fill)
                zz = dev_out(X.shape, torch.float32, fill) if case["noise"] and t is None else None
                engine.cfar_os_execute(d, xd, o, zz, N, ws, _lib.torch_stream_ptr())
                torch.cuda.synchronize()
                return o.cpu().numpy(), (None if zz is None else zz.cpu().numpy().astype(np.float64))
            ratio, z = call(None)
            ratio = ratio.astype(np.float64)
            hit = call(thr)[0] > 0.5 if case["thresh"] else None
        return dict(frames=[(ratio[i], None if z is None else z[i], None if hit is None else hit[i]) for i in range(len(order))],
                    whole=None)

    @staticmethod
    def check(case, f, got, want):
        from conftest import rel_err
        from test_gpu_cfar_os import TIGHT, bits, same, ulps
        ratio, z, hit = got
        w, x = want["frames"][f], inputs(case)[f]
        if case["dtype"] == "f32":          # test_exact_selection: the selection is exact, the plain ratio the IEEE quotient
            assert z is None or np.array_equal(bits(z), bits(w["z"])), f"frame {f}: the noise map differs from the oracle's"
            if case["scale"] == "plain":
                with np.errstate(divide="ignore", invalid="ignore"):
                    assert same(ratio, x / w["z"]), f"frame {f}: the plain ratio is not the float32 quotient"
            else:
                e = rel_err(ratio, w["ratio"])
                assert e < TIGHT, f"frame {f}: ratio {e:.3g}"
        else:                               # test_complex_input: hypotf on the load is the one inexact step
            assert z is None or ulps(z, w["z"]).max() <= 4, f"frame {f}: z {ulps(z, w['z']).max()} ulps"
            e = rel_err(ratio, w["ratio"])
            assert e < TIGHT, f"frame {f}: ratio {e:.3g}"
        if hit is not None:                 # test_placement_and_front_ends: thresholded == ratio > thresh
            with np.errstate(invalid="ignore"):
                assert hit.dtype == bool and np.array_equal(hit, ratio.astype(np.float32) > np.float32(want["thr"])), f"frame {f}: hits"


CfarOs.STRADDLE = {
    "cfar_os.TILE_ROWS": (lambda c: c["H"] > CfarOs.TILE_ROWS, {False, True}),
    "cfar_os.TILE_COLS": (lambda c: c["W"] > CfarOs.TILE_COLS, {False, True}),
    "cfar_os.fw parity": (lambda c: c["fw"] % 2, {0, 1}),
    "cfar_os.window wraps more than once": (lambda c: c["fw"] > min(c["H"], c["W"]), {False, True}),
    "cfar_os.rank": (lambda c: c["rank"], {"one", "nt", "default"}),
    "cfar_os.scale": (lambda c: c["scale"], {"reference", "plain"}),
    "cfar_os.input": (lambda c: c["dtype"], {"f32", "c64"}),
    "cfar_os.noise": (lambda c: c["noise"], {False, True}),
    "cfar_os.thresh": (lambda c: c["thresh"], {False, True}),
    "cfar_os.nframes": (lambda c: c["nframes"], {1, 2, 3}),
}


# ---- plots -----------------------------------------------------------------------------------------------------------------------
class Plots(Kind):
    name, header = "plots", "plot extraction"
    LDS_CELLS = 4096                        # PRC_PLOTS_LDS_CELLS of include/prcore.h: above, the lists sit in the workspace
    SMALL_CAPACITY = 3

    @staticmethod
    def draw(rng):
        H, W = pick(rng, [(9, 17), (24, 40), (33, 130), (32, 128), (37, 111), (40, 150), (40, 150)])
        nframes = int(rng.integers(1, 4))
        mc = pick(rng, ["auto", "lds", "all", "between"])
        return dict(kind="plots", H=H, W=W, density=pick(rng, [0.02, 0.3, 0.6, 0.85, 0.85]), connectivity=pick(rng, [4, 8]),
                    guards=pick(rng, [(0, 0), (0, 0), (8, 4), (3, 2)]), weight=pick(rng, ["none", "f32", "c64"]), nframes=nframes,
                    max_cells=mc if nframes > 1 or mc != "between" else "auto", capacity=pick(rng, ["auto", "small", "ample"]),
                    seed=int(rng.integers(1 << 30)))

    @staticmethod
    def nframes(case):
        return case["nframes"]

    @staticmethod
    def dense_frame(case):
        """the frame that detects in more cells than the others (max_cells 'between': it is over the bound)"""
        return 1 if case["max_cells"] == "between" else None

    @staticmethod
    def inputs(case):
        out = []
        for f in range(case["nframes"]):
            rng, shape = seeded(case, f), (case["H"], case["W"])
            stat = rng.random(shape).astype(np.float32)
            if f == Plots.dense_frame(case):
                stat += np.float32(0.5 * (1.0 - case["density"]) + 0.05)
            w = None
            if case["weight"] == "f32":
                w = rng.exponential(1.0, shape).astype(np.float32)
            elif case["weight"] == "c64":
                w = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)
            out.append((stat, w))
        return out

    @staticmethod
    def thresh(case):
        return 1.0 - case["density"]

    @staticmethod
    def expected(case):
        import plots_oracle as PO
        from test_gpu_plots import EXT
        g = case["guards"]
        frames = [PO.plots(s, Plots.thresh(case), EXT, w, case["connectivity"], g[0], g[1]) for s, w in inputs(case)]
        for w in frames:
            del w["labels"]
        cells = [w["ncells_total"] for w in frames]
        dense = Plots.dense_frame(case)
        mc = {"auto": None, "lds": Plots.LDS_CELLS, "all": case["H"] * case["W"],
              "between": max([c for f, c in enumerate(cells) if f != dense] + [1])}[case["max_cells"]]
        cap = {"auto": None, "small": Plots.SMALL_CAPACITY, "ample": 512}[case["capacity"]]
        return dict(frames=frames, max_cells=mc, capacity=cap)

    @staticmethod
    def over(case, want, f):
        return want["max_cells"] is not None and want["frames"][f]["ncells_total"] > want["max_cells"]

    @staticmethod
    def bounds(case, want, order):
        """(max_cells, capacity) the call ends up with: pinned, or what the sizing step arrives at for these frames"""
        mc, cap = want["max_cells"], want["capacity"]
        if mc is None:
            mc = max([Plots.LDS_CELLS] + [want["frames"][f]["ncells_total"] for f in order])
        if cap is None:
            cap = max([512] + [want["frames"][f]["count"] for f in order if not Plots.over(case, want, f)])
        return mc, cap

    @staticmethod
    def conditioned(case, want):
        dense = Plots.dense_frame(case)
        if dense is not None:
            assert Plots.over(case, want, dense) and not any(Plots.over(case, want, f) for f in range(case["nframes"]) if f != dense)

    @staticmethod
    def run(case, order, fill, plain, max_cells="case"):
        from passiveradar_amd import _lib
        from test_gpu_plots import EXT
        xs, want = inputs(case), expected(case)
        order = list(range(case["nframes"])) if order is None else order
        stat = np.stack([xs[f][0] for f in order])
        weight = None if case["weight"] == "none" else np.stack([xs[f][1] for f in order])
        kw = dict(connectivity=case["connectivity"], range_guard=case["guards"][0], doppler_guard=case["guards"][1])
        if fill is None and max_cells == "case":
            from passiveradar_amd.target_detection import extract_plots
            counts, meas, index, info, ncells = extract_plots(stat, Plots.thresh(case), EXT, weight=weight, return_info=True,
                                                              max_cells=want["max_cells"], capacity=want["capacity"], **kw)
        else:                               # prc_plots on caller-owned buffers: the workspace holds ``fill``, the outputs zeros
            import torch
            from passiveradar_amd import engine
            mc, cap = Plots.bounds(case, want, order)
            mc = mc if max_cells == "case" else max_cells
            N = stat.shape[0]
            d = engine.plots_desc(case["H"], case["W"], Plots.thresh(case), EXT, max_cells=mc, capacity=cap,
                                  complex_weight=case["weight"] == "c64", **kw)
            nws = engine.plots_workspace_bytes(d, N)
            ws = dev_bytes(nws, fill) if nws else None
            c, nc = dev_out((N,), torch.int32, fill), dev_out((N,), torch.int32, fill)
            cands = torch.zeros(N * cap * 32, dtype=torch.uint8, device="cuda")
            inf = torch.zeros(N * cap * 48, dtype=torch.uint8, device="cuda")
            engine.plots_execute(d, dev(stat), dev(weight), N, c, nc, cands, inf, ws, _lib.torch_stream_ptr())
            torch.cuda.synchronize()
            counts, ncells = c.cpu().numpy(), nc.cpu().numpy()
            rec = cands.cpu().numpy().view(_lib.TRACK_CAND_DTYPE).reshape(N, cap)
            meas = np.ascontiguousarray(np.stack((rec["range"], rec["doppler"], rec["strength"]), axis=1))
            index = np.ascontiguousarray(rec["index"])
            info = inf.cpu().numpy().view(_lib.PLOT_INFO_DTYPE).reshape(N, cap)
        frames = []
        for i in range(len(order)):
            k = min(int(counts[i]), meas.shape[2])
            untouched = not (meas[i][:, k:].any() or index[i][k:].any() or info[i][k:].view(np.uint8).any())
            frames.append((np.int32(counts[i]), np.int32(ncells[i]), meas[i][:, :k].copy(), index[i][:k].copy(), info[i][:k].copy(),
                           np.bool_(untouched)))
        return dict(frames=frames, whole=None)

    @staticmethod
    def check(case, f, got, want):
        from test_gpu_plots import check_frame
        count, ncells, meas, index, info, untouched = got
        w = want["frames"][f]
        assert untouched, f"frame {f}: a slot past the stored plots was written"
        if Plots.over(case, want, f):       # test_frame_over_max_cells: counts 0, the true ncells, nothing written
            assert count == 0 and ncells == w["ncells_total"], f"frame {f} over max_cells: counts {count}, ncells {ncells}"
            return
        held = min(want["max_cells"] or w["ncells_total"], case["H"] * case["W"])
        stack = tuple(np.asarray(v)[None] for v in (count, meas, index, info, ncells))
        check_frame(stack, 0, w, capacity=meas.shape[1] if want["capacity"] else None, scale=max(1.0, held / Plots.LDS_CELLS),
                    shape=(case["H"], case["W"]))
        assert meas.shape[1] == min(w["count"], want["capacity"] or w["count"]), f"frame {f}: {meas.shape[1]} plots stored"

    @staticmethod
    def extra_passes(case, base):
        """the other storage path (the same bytes on both): where every frame holds at most LDS_CELLS detections and the frame
        has more cells than that, max_cells = LDS_CELLS is the LDS path and max_cells = H W the workspace path"""
        want = expected(case)
        cells = [w["ncells_total"] for w in want["frames"]]
        if case["H"] * case["W"] <= Plots.LDS_CELLS or max(cells) > Plots.LDS_CELLS or case["max_cells"] == "between":
            return []
        mc = Plots.bounds(case, want, list(range(case["nframes"])))[0]
        other = case["H"] * case["W"] if mc <= Plots.LDS_CELLS else Plots.LDS_CELLS
        return [(f"max_cells {other}: the other storage path", Plots.run(case, None, 0x5A, False, max_cells=other)["frames"])]


def _plots_storage(c):
    want = expected(c)
    mc = Plots.bounds(c, want, list(range(c["nframes"])))[0]
    return min(mc, c["H"] * c["W"]) > Plots.LDS_CELLS


Plots.STRADDLE = {
    "plots.LDS_CELLS storage path": (_plots_storage, {False, True}),
    "plots.LDS_CELLS detections of a frame": (lambda c: {w["ncells_total"] > Plots.LDS_CELLS for w in expected(c)["frames"]},
                                              {False, True}),
    "plots.frame over max_cells": (lambda c: any(Plots.over(c, expected(c), f) for f in range(c["nframes"])), {False, True}),
    "plots.plots over capacity": (lambda c: any(w["count"] > (expected(c)["capacity"] or 1 << 30) for w in expected(c)["frames"]),
                                  {False, True}),
    "plots.connectivity": (lambda c: c["connectivity"], {4, 8}),
    "plots.guards": (lambda c: c["guards"] != (0, 0), {False, True}),
    "plots.weight": (lambda c: c["weight"], {"none", "f32", "c64"}),
}


# ---- tbd -------------------------------------------------------------------------------------------------------------------------
class Tbd(Kind):
    name, header = "tbd", "track-before-detect"
    FRAMES = 8                              # PRC_TBD_FRAMES of include/prcore.h: K of the shipped time-blocked form
    MAX_CODES = 255                         # (2 qd + 1)(2 qr + 1) <= 255

    @staticmethod
    def draw(rng):
        reach = pick(rng, [(0, 0), (1, 1), (1, 1), (2, 3), (1, 5), (2, 25), (7, 8)])
        big = (2 * reach[0] + 1) * (2 * reach[1] + 1) > 100      # the oracle visits every code per frame
        H, W = pick(rng, [(5, 7), (16, 64), (17, 65)] if big else [(5, 7), (16, 64), (17, 65), (33, 130), (9, 40), (40, 150)])
        N = pick(rng, [1, 2, 7, 8, 9] if big else [1, 2, 7, 8, 9, 13, 19])
        back = bool(rng.integers(4))
        return dict(kind="tbd", H=H, W=W, reach=reach, nframes=N, K=pick(rng, [None, None, 1, 2, 3, 5, 8, 32]),
                    band_rows=pick(rng, [None, None, 1, 2, 7, 4096]), alpha=pick(rng, [1.0, 0.9, 0.5]),
                    shift=pick(rng, ["none", "small", "beyond+", "beyond-", "extremes"]), prev=bool(rng.integers(2)), back=back,
                    clip=pick(rng, [None, 2.0]), guards=pick(rng, [(0, 0), (8, 4), (2, 1)]),
                    values=pick(rng, ["rayleigh", "rayleigh", "quantised", "special"]),
                    cut=int(rng.integers(1, N)) if N > 1 and rng.integers(2) else None,
                    depth=pick(rng, [1, 3, N, N + 4]) if back else None, seed=int(rng.integers(1 << 30)))

    @staticmethod
    def inputs(case):
        rng = seeded(case)
        N, H, W = case["nframes"], case["H"], case["W"]
        i32 = np.iinfo(np.int32)
        stat = rng.rayleigh(1.0, (N, H, W)).astype(np.float32)
        if case["values"] == "quantised":
            stat = rng.integers(0, 3, (N, H, W)).astype(np.float32)
        elif case["values"] == "special":
            flat = stat.reshape(N, -1)
            for v in (np.nan, np.inf, -np.inf):
                for f in range(N):
                    flat[f, rng.choice(H * W, 3, replace=False)] = v
        shifts = {"none": None, "small": rng.integers(-4, 5, H).astype(np.int32),
                  "beyond+": (W + case["reach"][1] + rng.integers(0, 3, H)).astype(np.int32),
                  "beyond-": (-(W + case["reach"][1]) - rng.integers(0, 3, H)).astype(np.int32),
                  "extremes": np.where(np.arange(H) % 3 == 0, i32.min, np.where(np.arange(H) % 3 == 1, i32.max, 1)).astype(np.int32)
                  }[case["shift"]]
        prev = rng.rayleigh(1.0, (H, W)).astype(np.float32) if case["prev"] else None
        ends = None
        if case["back"]:
            ends = [[int(rng.integers(N)), int(c)] for c in rng.choice(H * W, min(H * W, 12), replace=False)]
            ends += [[-1, 0], [N, 0], [0, -1], [0, H * W], [i32.max, 1], [N - 1, i32.min], [N - 1, H * W - 1], [0, 0]]
        return dict(stat=stat, shifts=shifts, prev=prev, ends=ends)

    @staticmethod
    def expected(case):
        import tbd_oracle as TO
        x = inputs(case)
        qd, qr = case["reach"]
        score, back = TO.tbd(x["stat"], qd, qr, case["alpha"], np.inf if case["clip"] is None else case["clip"], case["guards"][0],
                             case["guards"][1], x["shifts"], x["prev"])
        paths = TO.trace(back, x["ends"], case["depth"], qd, qr, x["shifts"]) if case["back"] else None
        return dict(score=score, back=back, paths=paths)

    @staticmethod
    def call(case, stat, prev, fill, plain):
        """one prc_tbd call as tests/test_gpu_tbd.py makes it: (score, back or None)"""
        import torch
        from passiveradar_amd import _lib, engine
        N, H, W = stat.shape
        d = engine.tbd_desc(H, W, case["alpha"], case["reach"][0], case["reach"][1], case["clip"], case["guards"][0], case["guards"][1])
        score = dev_out((N, H, W), torch.float32, fill)
        back = dev_out((N, H, W), torch.uint8, fill) if case["back"] else None
        engine.tbd_execute(d, dev(stat), dev(inputs(case)["shifts"]), dev(prev), N, score, back, _lib.torch_stream_ptr(),
                           None if plain else case["K"], None if plain else case["band_rows"])
        torch.cuda.synchronize()
        return score.cpu().numpy(), (back.cpu().numpy() if case["back"] else None)

    @staticmethod
    def run(case, order, fill, plain):
        from passiveradar_amd.target_detection import tbd_paths
        x = inputs(case)
        score, back = Tbd.call(case, x["stat"], x["prev"], fill, plain)
        paths = split = None
        if case["back"]:
            paths = tbd_paths(back, x["ends"], case["depth"], x["shifts"], doppler_reach=case["reach"][0], range_reach=case["reach"][1])
        if case["cut"] is not None:         # the stack split with prev carried over is the stack run whole
            a = Tbd.call(case, x["stat"][:case["cut"]], x["prev"], fill, plain)
            b = Tbd.call(case, x["stat"][case["cut"]:], a[0][-1], fill, plain)
            split = (np.concatenate((a[0], b[0])), np.concatenate((a[1], b[1])) if case["back"] else None)
        return dict(frames=[(score, back, paths, split)], whole=None)

    @staticmethod
    def check(case, f, got, want):
        import tbd_oracle as TO
        score, back, paths, split = got
        for what, (s, b) in (("whole", (score, back)),) + ((("split", split),) if split is not None else ()):
            assert TO.same_bits(s, want["score"]), \
                f"{what}: score differs in {int((s.view(np.uint32) != want['score'].view(np.uint32)).sum())} cell(s)"
            assert b is None or np.array_equal(b, want["back"]), f"{what}: back differs in {int((b != want['back']).sum())} cell(s)"
        assert paths is None or (paths.dtype == np.int32 and np.array_equal(paths, want["paths"])), "paths differ"


Tbd.STRADDLE = {
    "tbd.MAX_CODES reached": (lambda c: (2 * c["reach"][0] + 1) * (2 * c["reach"][1] + 1) == Tbd.MAX_CODES, {False, True}),
    "tbd.reach (0, 0)": (lambda c: c["reach"] == (0, 0), {False, True}),
    "tbd.FRAMES divides nframes": (lambda c: c["nframes"] % (c["K"] or Tbd.FRAMES) == 0, {False, True}),
    "tbd.one frame per launch": (lambda c: c["K"] == 1, {False, True}),
    "tbd.band rows": (lambda c: c["band_rows"], {None, 1}),
    "tbd.row_shift": (lambda c: c["shift"], {"none", "small", "beyond+", "beyond-"}),
    "tbd.prev": (lambda c: c["prev"], {False, True}),
    "tbd.back": (lambda c: c["back"], {False, True}),
    "tbd.clip": (lambda c: c["clip"] is None, {False, True}),
    "tbd.guards": (lambda c: c["guards"] != (0, 0), {False, True}),
}


# ---- track -----------------------------------------------------------------------------------------------------------------------
class Track(Kind):
    name, header = "track", "target tracking"
    MIN_H, MIN_W = 8, 17                    # prc_track_plan_create: below, the reference's mask slices go negative or overlap
    LDS_CAP = 4096                          # csrc/track.hip: the candidates one workgroup sorts in LDS
    EXT = [120.0, 60.0]

    @staticmethod
    def draw(rng):
        H, W = pick(rng, [(8, 17), (9, 17), (8, 18), (12, 40), (24, 40), (33, 130), (33, 130), (40, 150), (40, 150)])
        p = pick(rng, [0.0, 0.0, 100.0, 50.0, 99.8, 99.8, 90.0])
        return dict(kind="track", H=H, W=W, percentile=p, values=pick(rng, ["exponential", "exponential", "ties", "sparse"]),
                    capacity=pick(rng, ["auto", "below", "above"]), ntracks=pick(rng, [1, 3, 10]), nframes=int(rng.integers(1, 5)),
                    seed=int(rng.integers(1 << 30)))

    @staticmethod
    def nframes(case):
        return case["nframes"]

    @staticmethod
    def tracked(case):
        """the tracker runs on the lists where they are short enough for the restated tracker (a Python loop per candidate)"""
        return case["percentile"] >= 90.0

    @staticmethod
    def inputs(case):
        out = []
        H, W = case["H"], case["W"]
        for f in range(case["nframes"]):
            rng = seeded(case, f)
            x = rng.exponential(1.0, (H, W)).astype(np.float32)
            if case["values"] == "sparse":
                x[rng.random((H, W)) < 0.7] = 0.0
            if case["values"] == "ties":    # equal strongest cells and a plateau of equal ordinary ones
                for _ in range(4):
                    x[int(rng.integers(H)), int(rng.integers(W))] = 40.0
                x[rng.random((H, W)) < 0.2] = 1.5
            x[int(rng.integers(H)), min(W - 1, 8 + (3 * f) % max(W - 16, 1))] += 25.0      # something for a track to follow
            out.append(x)
        return out

    @staticmethod
    def expected(case):
        import tracker_oracle as T
        frames = [T.measure(x, Track.EXT, case["percentile"]) for x in inputs(case)]
        counts = [m["count"] for m in frames]
        cap = {"auto": None, "below": max(1, min(counts) // 2), "above": max(counts) + 3}[case["capacity"]]
        hist = None
        if Track.tracked(case):
            k = [min(c, cap or c) for c in counts]
            hist = T.history_arrays(T.track([(m["range"][:n], m["doppler"][:n]) for m, n in zip(frames, k)], case["ntracks"]))
        return dict(frames=frames, capacity=cap, hist=hist)

    @staticmethod
    def run(case, order, fill, plain):
        from passiveradar_amd.target_detection import _device_measure
        xs, want = inputs(case), expected(case)
        whole = order is None
        order = list(range(case["nframes"])) if order is None else order
        m = _device_measure(np.stack([xs[f] for f in order]), Track.EXT, case["ntracks"], capacity=want["capacity"],
                            percentile=case["percentile"])
        c = m.candidates()
        frames = []
        for i in range(len(order)):
            k = min(int(m.counts[i]), m.capacity)
            frames.append((np.int32(m.counts[i]), c[i]["index"][:k].copy(), c[i]["range"][:k].copy(), c[i]["doppler"][:k].copy(),
                           c[i]["strength"][:k].copy()))
        rec = None
        if whole and Track.tracked(case):
            r = m.run()
            rec = {k: r[k].copy() for k in ("status", "lifetime", "measurement", "estimate", "x", "P", "S", "history", "overflow")}
        return dict(frames=frames, whole=rec)

    @staticmethod
    def check(case, f, got, want):
        count, idx, rng_, dop, strength = got
        w = want["frames"][f]
        k = min(w["count"], want["capacity"] or w["count"])
        assert count == w["count"], f"frame {f}: {count} candidates, the restatement has {w['count']}"
        assert np.array_equal(idx, w["idx"][:k]), f"frame {f}: indices"
        assert np.array_equal(rng_, w["range"][:k]) and np.array_equal(dop, w["doppler"][:k]), f"frame {f}: coordinates"
        np.testing.assert_allclose(strength, w["strength"][:k], rtol=1e-12, atol=0, err_msg=f"frame {f}: strengths")

    @staticmethod
    def check_whole(case, got, want):
        h = want["hist"]
        assert np.array_equal(got["status"], h["status"]) and np.array_equal(got["lifetime"], h["lifetime"]), "status / lifetime"
        assert np.array_equal(got["history"].astype(np.float64), h["hist"]), "measurement history"
        np.testing.assert_allclose(got["estimate"], h["estimate"], rtol=1e-9, atol=1e-9, err_msg="estimate")
        over = np.array([m["count"] > (want["capacity"] or m["count"]) for m in want["frames"]], dtype=np.int32)
        assert np.array_equal(got["overflow"][:, 0], over), "overflow flags"


def _track_counts(c):
    want = expected(c)
    return want, [m["count"] for m in want["frames"]]


Track.STRADDLE = {
    "track.MIN_H": (lambda c: c["H"] == Track.MIN_H, {False, True}),
    "track.MIN_W": (lambda c: c["W"] == Track.MIN_W, {False, True}),
    "track.percentile": (lambda c: "mid" if 0.0 < c["percentile"] < 100.0 else c["percentile"], {0.0, 100.0, "mid"}),
    "track.capacity below the count": (lambda c: any(n > (_track_counts(c)[0]["capacity"] or n) for n in _track_counts(c)[1]),
                                       {False, True}),
    "track.LDS_CAP": (lambda c: {n > Track.LDS_CAP for n in _track_counts(c)[1]}, {False, True}),
    "track.planted ties": (lambda c: c["values"] == "ties", {False, True}),
    "track.tracker run": (Track.tracked, {False, True}),
}


# ---- strack ----------------------------------------------------------------------------------------------------------------------
class Strack(Kind):
    name, header = "strack", "single-target tracker"
    MASK = (250, 260)                       # the Doppler columns s[:, 250:260] the reference zeroes (Python slice rules)
    FIELDS = ("lock_mode", "measurement_idx", "measurement", "estimate", "x", "P", "S")
    EXT = (375.0, 234.0)

    @staticmethod
    def draw(rng):
        N = int(rng.integers(6, 19))
        return dict(kind="strack", H=pick(rng, [240, 249, 250, 251, 255, 259, 260, 261, 270]), W=pick(rng, [17, 20, 24, 33]),
                    dtype=pick(rng, ["f32", "f64"]), nframes=N, cut=int(rng.integers(1, N)), fade=bool(rng.integers(2)),
                    seed=int(rng.integers(1 << 30)))

    @staticmethod
    def inputs(case):
        """exponential clutter and a target that wanders in range and Doppler (and fades out for a while): (H, W, N)"""
        rng = seeded(case)
        N, H, W = case["nframes"], case["H"], case["W"]
        f = rng.exponential(1.0, (N, H, W))
        r, c = W / 2.0, H / 2.0 + 20.0
        for i in range(N):
            r = min(max(r + rng.normal(0, 0.4), 8.5), W - 9.5)
            c = min(max(c + rng.normal(0, 1.0), 10), H - 10)
            if not (case["fade"] and N // 3 <= i < N // 3 + 3):
                f[i, H - 1 - int(round(c)), int(round(r))] += 60.0
        return np.ascontiguousarray(np.moveaxis(f, 0, 2)).astype(np.float32 if case["dtype"] == "f32" else np.float64)

    @staticmethod
    def expected(case):
        import simple_tracker_oracle as O
        with np.errstate(all="ignore"):
            return O.simple_target_tracker(inputs(case), *Strack.EXT)

    @staticmethod
    def conditioned(case, want):
        assert np.abs(want["badness"] - 12).min() > 1e-6, "a frame's badness sits on the lock threshold"

    @staticmethod
    def arrays(h):
        ks = h["kalman_state"]
        return dict(lock_mode=h["lock_mode"], measurement=h["measurement"], measurement_idx=h["measurement_idx"],
                    estimate=h["estimate"], x=ks["x"], P=ks["P"].reshape(-1, 16), S=ks["S"].reshape(-1, 4))

    @staticmethod
    def run(case, order, fill, plain):
        from passiveradar_amd.target_detection import simple_target_tracker
        x, cut = inputs(case), case["cut"]
        whole = simple_target_tracker(x, *Strack.EXT)
        a = simple_target_tracker(x[:, :, :cut], *Strack.EXT)
        b = simple_target_tracker(x[:, :, cut:], *Strack.EXT, state=a[-1])
        w, s = Strack.arrays(whole), Strack.arrays(np.concatenate((a, b)))
        return dict(frames=[tuple(w[k] for k in Strack.FIELDS) + tuple(s[k] for k in Strack.FIELDS)], whole=None)

    @staticmethod
    def check(case, f, got, want):
        from test_simple_tracker_host import check_strack
        n = len(Strack.FIELDS)
        check_strack(dict(zip(Strack.FIELDS, got[:n])), want)
        for k, a, b in zip(Strack.FIELDS, got[:n], got[n:]):      # test_resumed_run_equals_one_run
            assert np.array_equal(a, b), f"resumed at frame {case['cut']}: {k} differs from the one call"


Strack.STRADDLE = {
    "strack.MASK begins inside the frame": (lambda c: c["H"] > Strack.MASK[0], {False, True}),
    "strack.MASK ends inside the frame": (lambda c: c["H"] >= Strack.MASK[1], {False, True}),
    "strack.dtype": (lambda c: c["dtype"], {"f32", "f64"}),
}


# ---- persistence -----------------------------------------------------------------------------------------------------------------
class Persistence(Kind):
    name, header = "persistence", "persistence"
    TERMS_PER_LAUNCH = 256                  # PRC_PERSISTENCE_TERMS_PER_LAUNCH: with more terms the launches chain through out

    @staticmethod
    def draw(rng):
        out = pick(rng, ["f64", "f64", "f32"])
        long = out == "f64" and bool(rng.integers(2))
        L = pick(rng, [258, 300]) if long else int(rng.integers(1, 40))
        hold = pick(rng, [257, 258, 300, 1000]) if long else pick(rng, [1, 2, 5, 20, 255, 256])
        where = pick(rng, ["first", "last", "all", "middle"])
        kc = L if where == "all" else int(rng.integers(1, min(L, 4) + 1))
        kf = {"first": 0, "all": 0, "last": L - kc, "middle": (L - kc) // 2}[where]
        return dict(kind="persistence", H=pick(rng, [1, 3, 7]), W=pick(rng, [1, 5, 33]) if long else pick(rng, [1, 5, 33, 150]),
                    L=L, hold=hold, decay=pick(rng, [0.9, 0.5, -0.5, 0.999, 1.0]), k_first=kf, k_count=min(kc, 6) if long else kc,
                    in_dtype=pick(rng, ["f32", "f64"]), out_dtype=out, seed=int(rng.integers(1 << 30)))

    @staticmethod
    def nframes(case):
        return case["k_count"]

    @classmethod
    def orders(cls, case):
        """an output frame alone, and the range shortened at either end (output frames are a contiguous range of k)"""
        n = case["k_count"]
        return [[j] for j in range(n)] + ([list(range(1, n)), list(range(n - 1))] if n > 1 else [])

    @staticmethod
    def inputs(case):
        x = seeded(case).exponential(1.0, (case["H"], case["W"], case["L"]))
        return x.astype(np.float32 if case["in_dtype"] == "f32" else np.float64)

    @staticmethod
    def expected(case):
        import simple_tracker_oracle as O
        x = inputs(case)
        out = [O.persistence(x, case["k_first"] + j, case["hold"], case["decay"], weak=True) for j in range(case["k_count"])]
        return [o.astype(np.float32) if case["out_dtype"] == "f32" else o for o in out]

    @staticmethod
    def run(case, order, fill, plain):
        import torch
        from passiveradar_amd import _lib, plotting_tools
        x = inputs(case)
        order = list(range(case["k_count"])) if order is None else order
        assert order == list(range(order[0], order[0] + len(order)))
        frames = dev(np.moveaxis(x, 2, 0))                           # [L, H, W]
        elems, n = case["H"] * case["W"], len(order)
        odt = torch.float32 if case["out_dtype"] == "f32" else torch.float64
        out = dev_out((n, elems), odt, fill)
        code = lambda d: _lib.REAL_F32 if d == "f32" else _lib.REAL_F64      # noqa: E731
        plotting_tools._run(frames.data_ptr(), code(case["in_dtype"]), elems, case["L"], case["k_first"] + order[0], n, case["hold"],
                            case["decay"], out.data_ptr(), code(case["out_dtype"]), _lib.torch_stream_ptr())
        torch.cuda.synchronize()
        got = out.cpu().numpy().reshape(n, case["H"], case["W"])
        return dict(frames=[(got[i],) for i in range(n)], whole=None)

    @staticmethod
    def check(case, f, got, want):
        a, b = got[0], want[f]
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), f"k = {case['k_first'] + f}: {int((a != b).sum())} cell(s) differ"


Persistence.STRADDLE = {
    "persistence.TERMS_PER_LAUNCH": (lambda c: min(c["hold"], c["k_first"] + c["k_count"]) > Persistence.TERMS_PER_LAUNCH, {False, True}),
    "persistence.k_first at the start": (lambda c: c["k_first"] == 0, {False, True}),
    "persistence.k_count to the end": (lambda c: c["k_first"] + c["k_count"] == c["L"], {False, True}),
    "persistence.dtypes": (lambda c: (c["in_dtype"], c["out_dtype"]), {("f32", "f32"), ("f32", "f64"), ("f64", "f32"), ("f64", "f64")}),
}


# ---- display ---------------------------------------------------------------------------------------------------------------------
class Display(Kind):
    name, header = "display", "display frames"

    @staticmethod
    def draw(rng):
        return dict(kind="display", shape=pick(rng, [(1, 1), (2, 1), (1, 2), (3, 5), (37, 23), (33, 64), (40, 150), (100, 45)]),
                    p=pick(rng, [(35, 99), (0, 100), (50, 50), (0, 0), (100, 100), (12.5, 87.25), (99.9, 0.1)]),
                    hi_scale=pick(rng, [1.5, 1.0, 2.0]), dtype=pick(rng, ["f32", "f64"]), orient=pick(rng, ["plot", "stored"]),
                    values=pick(rng, ["dense", "dense", "two_values", "constant", "half_zero", "one_inf", "negative"]),
                    lut=pick(rng, ["gnuplot2", "table"]), nframes=int(rng.integers(1, 4)), seed=int(rng.integers(1 << 30)))

    @staticmethod
    def nframes(case):
        return case["nframes"]

    @staticmethod
    def inputs(case):
        out = []
        for f in range(case["nframes"]):
            rng, shape = seeded(case, f), case["shape"]
            x = rng.exponential(1.0 + f, shape)
            if case["values"] == "two_values":
                x = np.where(rng.random(shape) < 0.3, 2.5, -1.25)
            elif case["values"] == "constant":
                x = np.full(shape, 4.25 + f)
            elif case["values"] == "half_zero":
                x[rng.random(shape) < 0.5] = 0.0
            elif case["values"] == "one_inf":
                x.flat[int(rng.integers(x.size))] = np.inf
            elif case["values"] == "negative":
                x = rng.standard_normal(shape) * 3.0 - 1.0
            out.append(x.astype(np.float32 if case["dtype"] == "f32" else np.float64))
        table = np.random.default_rng(3).integers(0, 256, (256, 4), dtype=np.uint8) if case["lut"] == "table" else None
        return dict(frames=out, lut=table)

    @staticmethod
    def expected(case):
        import display_oracle as D
        x = inputs(case)
        out = []
        for f in x["frames"]:
            f64 = f.astype(np.float64)                               # a float32 frame is its values widened
            lim = D.limits(f64, case["p"][0], case["p"][1], case["hi_scale"])
            out.append((lim, D.render(f64, lut=x["lut"], lim=lim, orient=case["orient"])))
        return out

    @staticmethod
    def run(case, order, fill, plain):
        from passiveradar_amd.plotting_tools import display_limits, render_frames
        x = inputs(case)
        order = list(range(case["nframes"])) if order is None else order
        X = np.stack([x["frames"][f] for f in order], axis=2)        # (H, W, L) as the scripts hold it
        lim = display_limits(X, case["p"][0], case["p"][1], case["hi_scale"])
        px = render_frames(X, lut=x["lut"], p_lo=case["p"][0], p_hi=case["p"][1], hi_scale=case["hi_scale"], orient=case["orient"])
        return dict(frames=[(lim[i], px[i]) for i in range(len(order))], whole=None)

    @staticmethod
    def check(case, f, got, want):
        lim, px = got
        wl, wp = want[f]
        assert lim.dtype == np.float64 and np.array_equal(lim, wl, equal_nan=True), f"frame {f}: limits {lim} against {wl}"
        assert px.dtype == np.uint8 and px.shape == wp.shape and np.array_equal(px, wp), \
            f"frame {f}: {int((px != wp).any(axis=-1).sum())} pixel(s) differ"


Display.STRADDLE = {
    "display.frame of one cell": (lambda c: c["shape"][0] * c["shape"][1] == 1, {False, True}),
    "display.frame of two cells": (lambda c: c["shape"][0] * c["shape"][1] == 2, {False, True}),
    "display.odd frame": (lambda c: (c["shape"][0] * c["shape"][1]) % 2 == 1 and c["shape"] != (1, 1), {False, True}),
    "display.percentile 0": (lambda c: 0 in c["p"], {False, True}),
    "display.percentile 100": (lambda c: 100 in c["p"], {False, True}),
    "display.dtype": (lambda c: c["dtype"], {"f32", "f64"}),
    "display.orient": (lambda c: c["orient"], {"plot", "stored"}),
    "display.equal values": (lambda c: c["values"] in ("two_values", "constant"), {False, True}),
    "display.a frame holding Inf": (lambda c: c["values"] == "one_inf", {False, True}),
}


# ---- welch -----------------------------------------------------------------------------------------------------------------------
class Welch(Kind):
    name, header = "welch", "Welch spectra"
    NFFTS = (64, 128, 256, 512, 1024, 2048, 4096, 8192)      # every shipped transform length
    FS = 2.4e6

    @staticmethod
    def draw(rng):
        nfft = pick(rng, list(Welch.NFFTS))
        ov = pick(rng, ["none", "half", "all_but_one", "odd"])
        noverlap = {"none": 0, "half": nfft // 2, "all_but_one": nfft - 1, "odd": 37}[ov]
        hop = nfft - noverlap
        length = pick(rng, ["short", "exact", "fits", "misses", "ragged"])
        nseg = int(rng.integers(2, 7))
        n = {"short": nfft - int(rng.integers(1, 40)), "exact": nfft, "fits": nfft + (nseg - 1) * hop,
             "misses": nfft + (nseg - 1) * hop - 1, "ragged": nfft + (nseg - 1) * hop + int(rng.integers(0, hop))}[length]
        op = pick(rng, ["psd", "psd", "csd", "specgram", "specgram"])
        segs = 1 if n < nfft else (n - nfft) // hop + 1
        return dict(kind="welch", nfft=nfft, noverlap=noverlap, n=n, length=length, detrend=pick(rng, ["none", "mean"]),
                    input=pick(rng, ["c64", "c64", "int8"]) if op != "csd" else "c64", op=op,
                    navg=pick(rng, [n_ for n_ in (0, 1, 2) if n_ <= segs]) if op == "specgram" else 0, step=pick(rng, [1, 1, 2]),
                    nch=int(rng.integers(1, 4)), seed=int(rng.integers(1 << 30)))

    @staticmethod
    def nframes(case):
        return case["nch"]

    @staticmethod
    def inputs(case):
        """per channel: what is handed to the entry point (every other sample of it is the channel when step == 2: the ones
        between hold NaN, or 127 in a raw recording) and the complex64 samples it stands for, as the oracle takes them"""
        import psd_oracle as P
        out = []
        n, step = case["n"], case["step"]
        for c in range(case["nch"]):
            s = int(case["seed"]) % 100000 + 7 * c
            if case["input"] == "int8":
                raw, z = P.int8_raw(n, s)
                given = raw
                if step == 2:
                    given = np.full(4 * n, 127, np.int8)
                    given.reshape(-1, 2, 2)[:, 0, :] = raw.reshape(-1, 2)
            else:
                z = P.white(n, s)
                given = z
                if step == 2:
                    given = np.full(2 * n, np.nan, np.complex64)
                    given[0::2] = z
            y = gy = None
            if case["op"] == "csd":
                y = (np.roll(z, 5) * (0.5 - 0.2j) + 0.1 * P.white(n, s + 1)).astype(np.complex64)
                gy = y
                if step == 2:
                    gy = np.full(2 * n, np.nan, np.complex64)
                    gy[0::2] = y
            out.append(dict(given=given, z=z, given_y=gy, y=y))
        return out

    @staticmethod
    def expected(case):
        import psd_oracle as P
        return [P.welch(ch["z"], ch["y"], case["nfft"], Welch.FS, case["detrend"], None, case["noverlap"], True, case["navg"])
                for ch in inputs(case)]

    @staticmethod
    def run(case, order, fill, plain):
        from passiveradar_amd import spectral
        chs = inputs(case)
        order = list(range(case["nch"])) if order is None else order
        stack = lambda key: np.stack([chs[c][key] for c in order]) if len(order) > 1 else chs[order[0]][key]      # noqa: E731
        kw = dict(NFFT=case["nfft"], Fs=Welch.FS, detrend=case["detrend"], noverlap=case["noverlap"], raw=case["input"] == "int8",
                  step=case["step"])
        if case["op"] == "psd":
            out = spectral.psd(stack("given"), **kw)[0]
        elif case["op"] == "csd":
            out = spectral.csd(stack("given"), stack("given_y"), **kw)[0]
        else:
            out = spectral.specgram(stack("given"), navg=case["navg"], **kw)[0]
            out = np.swapaxes(out, -1, -2)                           # [.., rows, nfft], as the oracle lays it out
        out = np.asarray(out)
        if len(order) == 1:
            out = out[None]
        return dict(frames=[(np.ascontiguousarray(out[i]).reshape(-1, case["nfft"]),) for i in range(len(order))], whole=None)

    @staticmethod
    def check(case, f, got, want):
        from test_gpu_psd import DB_BAR, REL_BAR, errors
        g, w = got[0], want[f]
        assert g.shape == w.shape and g.dtype == w.dtype, f"channel {f}: {g.shape} {g.dtype} against {w.shape} {w.dtype}"
        if case["op"] == "csd":
            e = float(np.abs(g - w).max() / np.abs(w).max())
            assert e <= REL_BAR, f"channel {f}: csd {e:.3g}"
        else:
            rel, db = errors(g, w)
            assert rel <= REL_BAR and db <= DB_BAR, f"channel {f}: rel {rel:.3g}, {db:.3g} dB"


Welch.STRADDLE = {
    "welch.NFFTS": (lambda c: c["nfft"], set(Welch.NFFTS)),
    "welch.noverlap": (lambda c: "none" if c["noverlap"] == 0 else "half" if c["noverlap"] == c["nfft"] // 2 else
                       "all_but_one" if c["noverlap"] == c["nfft"] - 1 else "odd", {"none", "half", "all_but_one"}),
    "welch.length": (lambda c: c["length"], {"short", "exact", "fits", "misses"}),
    "welch.detrend": (lambda c: c["detrend"], {"none", "mean"}),
    "welch.input": (lambda c: c["input"], {"c64", "int8"}),
    "welch.op": (lambda c: c["op"], {"psd", "csd", "specgram"}),
    "welch.navg": (lambda c: c["navg"] if c["op"] == "specgram" else None, {0, 1, 2}),
    "welch.step": (lambda c: c["step"], {1, 2}),
}


# ---- preproc ---------------------------------------------------------------------------------------------------------------------
class Preproc(Kind):
    name, header = "preproc", "FIR decimator and the rest of signal_utils.py"
    TILE_MAX_Q = 59                         # PRC_FIRDEC_TILE_MAX_Q: the last q of decimate's filter on the LDS-tile form
    TILE_OUTPUTS = 256                      # csrc/preproc.hip FD_TO: outputs per workgroup of the tile form
    FS = 2.4e6

    @staticmethod
    def draw(rng):
        op = pick(rng, ["decimate", "decimate", "decimate", "channel", "channel", "shift", "normalize"])
        c = dict(kind="preproc", op=op)
        if op in ("decimate", "channel"):
            q = pick(rng, [2, 3, 10, 58, 59, 60, 61, 97])
            m = pick(rng, [1, 37, Preproc.TILE_OUTPUTS - 1, Preproc.TILE_OUTPUTS, Preproc.TILE_OUTPUTS + 1, 300])
            n = max(1, m * q - int(rng.integers(0, q)))              # ceil(n / q) = m outputs
            c.update(q=q, n=n)
            if op == "decimate":
                c.update(ncols=int(rng.integers(1, 4)))
            else:
                c.update(raw=pick(rng, ["int8", "uint8", "int16", "float32"]), odd=bool(rng.integers(2)), fc=pick(rng, [1e5, -2.5e5, 5e4]))
        elif op == "shift":
            n = int(rng.integers(2, 3000))
            c.update(n=n, by=(0, n, -n, n + 3, -(n + 3), 1, -1, n - 1, -(n - 1), n // 2), dtype=pick(rng, ["c64", "i8x3"]))
        else:
            c.update(shape=pick(rng, [(1,), (7,), (3, 4), (255,), (256,), (257,), (5000,)]), dtype=pick(rng, ["float32", "complex64"]))
        c.update(seed=int(rng.integers(1 << 30)))
        return c

    @staticmethod
    def nframes(case):
        return case.get("ncols", 1)

    @staticmethod
    def inputs(case):
        import preproc_oracle as O
        s = int(case["seed"])
        if case["op"] == "decimate":
            return O.white(case["n"], s, case["ncols"])
        if case["op"] == "channel":
            return O.raw_input(case["raw"], 2 * case["n"] + case["odd"], s)
        if case["op"] == "shift":
            return O.white(case["n"], s) if case["dtype"] == "c64" else O.raw_int8(3 * case["n"], s).reshape(case["n"], 3)
        z = O.white(int(np.prod(case["shape"])), s).reshape(case["shape"])
        return (z if case["dtype"] == "complex64" else z.real).astype(case["dtype"])

    @staticmethod
    def expected(case):
        import preproc_oracle as O
        x = inputs(case)
        if case["op"] == "decimate":
            y = O.decimate(x, case["q"])
            return [y[:, c] for c in range(case["ncols"])]
        if case["op"] == "channel":
            return [O.channel_preprocessing(x, case["q"], case["fc"], Preproc.FS)]
        return [tuple(O.shift(x, k) for k in case["by"]) if case["op"] == "shift" else O.normalize(x)]

    @staticmethod
    def run(case, order, fill, plain):
        from passiveradar_amd import signal_utils as S
        x = inputs(case)
        if case["op"] == "decimate":
            order = list(range(case["ncols"])) if order is None else order
            y = S.decimate(np.ascontiguousarray(x[:, order]) if len(order) > 1 else np.ascontiguousarray(x[:, order[0]]), case["q"])
            y = y[:, None] if y.ndim == 1 else y
            return dict(frames=[(np.ascontiguousarray(y[:, i]),) for i in range(len(order))], whole=None)
        if case["op"] == "channel":
            return dict(frames=[(S.channel_preprocessing(x, case["q"], case["fc"], Preproc.FS),)], whole=None)
        if case["op"] == "shift":
            return dict(frames=[tuple(np.array(S.shift(x, k)) for k in case["by"])], whole=None)
        return dict(frames=[(S.normalize(x),)], whole=None)

    @staticmethod
    def check(case, f, got, want):
        from conftest import rel_err
        from test_gpu_preproc import BAR, NORM_BAR
        if case["op"] == "shift":
            for k, g, w in zip(case["by"], got, want[f]):
                assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g, w), f"shift by {k} is not exact"
            return
        g, w = got[0], want[f]
        assert g.shape == w.shape and g.dtype == w.dtype, f"{g.shape} {g.dtype} against {w.shape} {w.dtype}"
        e = rel_err(g, w)
        bar = NORM_BAR if case["op"] == "normalize" else BAR
        assert e <= bar, f"column {f}: {e:.3g} (bar {bar:g})"


Preproc.STRADDLE = {
    "preproc.TILE_MAX_Q": (lambda c: c["q"] > Preproc.TILE_MAX_Q if "q" in c else None, {False, True}),
    "preproc.TILE_OUTPUTS": (lambda c: -(-c["n"] // c["q"]) > Preproc.TILE_OUTPUTS if "q" in c else None, {False, True}),
    "preproc.op": (lambda c: c["op"], {"decimate", "channel", "shift", "normalize"}),
    "preproc.shift": (lambda c: {"zero" if k == 0 else "whole" if abs(k) == c["n"] else "beyond" if abs(k) > c["n"] else "inside"
                                 for k in c["by"]} if c["op"] == "shift" else None, {"zero", "whole", "beyond", "inside"}),
}


# ---- gal -------------------------------------------------------------------------------------------------------------------------
class Gal(Kind):
    name, header = "gal", "GAL_JPE"
    LANES = 64                              # csrc/gal.hip: ceil(D / 64) delay-line elements per lane (the kernel's template argument)
    CONSECUTIVE = 8                         # ... instantiated for 1 .. 8, then 10, 12, 14, ...: above 8 a count may be rounded up
    ROW_FORM_LATTICE = 64                   # lattice_len <= 64: the row form (one lattice row); above: the lattice kernel
    FAST_MAX = 2048                         # GAL_FAST_MAX: above, one workgroup per stream with its state in the workspace
    PEEK = 10

    @staticmethod
    def draw(rng):
        D = pick(rng, [1, 2, 63, 64, 65, 125, 128, 129, 320, 509, 512, 513, 577, 640, 700, Gal.FAST_MAX, Gal.FAST_MAX + 52])
        L = pick(rng, [1, min(D, 8), min(D, 64), min(D, 65), max(D // 2, 1), D])
        n = pick(rng, [Gal.PEEK + 2, Gal.PEEK + 3, 64, 260, 300 if D > 128 else 700])
        return dict(kind="gal", D=D, L=L, n=n, nstreams=pick(rng, [1, 1, 2, 5]), gap=pick(rng, [0, 33]),
                    mu=pick(rng, [(2e-3, 2e-2), (1e-3, 1e-2)]),
                    seed=int(rng.integers(1 << 30)))

    @staticmethod
    def nframes(case):
        return case["nstreams"]

    @staticmethod
    def inputs(case):
        from passiveradar_amd import scene
        out = []
        for s in range(case["nstreams"]):
            ref, srv = scene.make_ar2_scene(max(case["n"], 64), 262144.0, 64, int(case["seed"]) % 100000 + s)
            out.append((ref[:case["n"]].copy(), srv[:case["n"]].copy()))
        return out

    @staticmethod
    def expected(case):
        from gal_oracle import gal_jpe
        return [gal_jpe(r, s, case["L"], case["D"], case["mu"][0], case["mu"][1], Gal.PEEK, np.complex64, True) for r, s in inputs(case)]

    @staticmethod
    def run(case, order, fill, plain):
        import torch
        from passiveradar_amd import engine
        xs = inputs(case)
        order = list(range(case["nstreams"])) if order is None else order
        ns, n, D = len(order), case["n"], case["D"]
        stride, ostride = n + case["gap"], n + (case["gap"] and case["gap"] - 16)
        host = np.full((2, ns, stride), np.nan, np.complex64)        # the gaps hold NaN: nothing outside a stream is read
        for i, f in enumerate(order):
            host[0, i, :n], host[1, i, :n] = xs[f]
        out = dev_out((ns, ostride), torch.complex64, fill)
        kb, hb = dev_out((ns, D), torch.complex64, fill), dev_out((ns, D), torch.complex64, fill)
        wsb = engine.gal_workspace_bytes(D, ns)
        ws = dev_bytes(wsb, fill) if wsb else None
        engine.gal_execute(dev(host[0]), dev(host[1]), out, n, case["L"], D, case["mu"][0], case["mu"][1], Gal.PEEK, kb, hb, ns, stride,
                           ostride, ws)
        torch.cuda.synchronize()
        o, k, h = out.cpu().numpy(), kb.cpu().numpy(), hb.cpu().numpy()
        return dict(frames=[(o[i, :n].copy(), k[i].copy(), h[i].copy(), untouched(o[i, n:], fill)) for i in range(ns)], whole=None)

    @staticmethod
    def check(case, f, got, want):
        from conftest import rel_err
        err = lambda a, b: rel_err(a, b) if np.any(b) else float(np.abs(a).max())      # noqa: E731
        out, k, h, gap = got
        eo, ek, eh = want[f]
        n = case["n"]
        assert gap, f"stream {f}: out was written beyond its n elements"
        assert not np.any(out[max(n - Gal.PEEK - 1, 0):]), f"stream {f}: out is not zero where the reference never writes"
        assert k[0] == 0 and not np.any(k[case["L"]:]), f"stream {f}: k outside the lattice"
        e = (err(out, eo), err(k, ek), err(h, eh))
        assert e[0] <= 1e-4 and e[1] <= 2e-4 and e[2] <= 2e-4, f"stream {f}: out {e[0]:.3g}, k {e[1]:.3g}, h {e[2]:.3g}"


Gal.STRADDLE = {
    "gal.LANES": (lambda c: c["D"] > Gal.LANES, {False, True}),
    "gal.CONSECUTIVE": (lambda c: -(-c["D"] // Gal.LANES) > Gal.CONSECUTIVE, {False, True}),
    "gal.an element count that is rounded up": (lambda c: -(-c["D"] // Gal.LANES) in (9, 11), {False, True}),
    "gal.ROW_FORM_LATTICE": (lambda c: c["L"] > Gal.ROW_FORM_LATTICE and c["D"] <= Gal.FAST_MAX, {False, True}),
    "gal.FAST_MAX": (lambda c: c["D"] > Gal.FAST_MAX, {False, True}),
    "gal.lattice": (lambda c: "one" if c["L"] == 1 else "all" if c["L"] == c["D"] else "some", {"one", "all", "some"}),
    "gal.n barely above the minimum": (lambda c: c["n"] <= Gal.PEEK + 3, {False, True}),
    "gal.several streams": (lambda c: c["nstreams"] > 1, {False, True}),
}


# ---- ls_svd ----------------------------------------------------------------------------------------------------------------------
class LsSvd(Kind):
    name, header = "ls_svd", "LS_Filter_SVD"
    LAG_GROUP = 64                          # csrc/ls_svd.hip: lags per group of the correlation (SVD_LG groups per pass)
    TILE = 1024                             # SVD_TILE: samples staged per pass

    @staticmethod
    def draw(rng):
        L, peek = pick(rng, [(1, 0), (2, 0), (1, 1), (3, 0), (16, 10), (17, 10), (32, 10), (32, 31), (32, 32), (32, 33), (22, 0)])
        T = L + peek
        n = pick(rng, [T + 1, 63, 257, 1021, 1023, 1024, 1025, 2048])
        return dict(kind="ls_svd", n=max(n, T + 1), L=L, peek=peek, nblocks=int(rng.integers(1, 4)), gap=pick(rng, [0, 37]),
                    ref=pick(rng, ["white", "white", "ar1"]), seed=int(rng.integers(1 << 30)))

    @staticmethod
    def nframes(case):
        return case["nblocks"]

    @staticmethod
    def inputs(case):
        out = []
        n, T = case["n"], case["L"] + case["peek"]
        for b in range(case["nblocks"]):
            rng = seeded(case, b)
            ref = cwhite(rng, n)
            if case["ref"] == "ar1":
                w = ref.astype(np.complex128)
                for i in range(1, n):
                    w[i] += 0.7 * w[i - 1]
                ref = (w * math.sqrt(1.0 - 0.49)).astype(np.complex64)
            h0 = np.zeros(n, np.complex128)
            h0[:T] = cwhite(rng, T) * np.exp(-np.arange(T) / 6.0)
            clutter = np.fft.ifft(np.fft.fft(np.roll(ref.astype(np.complex128), -case["peek"])) * np.fft.fft(h0))
            out.append((ref, (clutter + 0.05 * cwhite(rng, n)).astype(np.complex64)))
        return out

    @staticmethod
    def expected(case):
        from ls_svd_oracle import ls_filter_svd
        out = []
        for ref, srv in inputs(case):
            info = {}
            o, t = ls_filter_svd(ref, srv, case["L"], case["peek"], None, info)
            out.append(dict(out=o, taps=t, sv=info["sv"], kept=info["kept"], cut=info["cut"]))
        return out

    @staticmethod
    def conditioned(case, want):
        for w in want:                      # no singular value of the float64 oracle within a factor 10 of the cut
            assert not np.any((w["sv"] > w["cut"] / 10.0) & (w["sv"] < w["cut"] * 10.0)), "a singular value sits near the rcond cut"

    @staticmethod
    def run(case, order, fill, plain):
        import torch
        from passiveradar_amd import engine
        xs = inputs(case)
        order = list(range(case["nblocks"])) if order is None else order
        nb, n, L, peek = len(order), case["n"], case["L"], case["peek"]
        T, stride, ostride = L + peek, n + case["gap"], n + (case["gap"] and case["gap"] - 16)
        host = np.full((2, nb, stride), np.nan, np.complex64)
        for i, f in enumerate(order):
            host[0, i, :n], host[1, i, :n] = xs[f]
        out = dev_out((nb, ostride), torch.complex64, fill)
        taps, sv = dev_out((nb, T), torch.complex128, fill), dev_out((nb, T), torch.float64, fill)
        info = dev_out((nb, 3), torch.int32, fill)
        ws = dev_bytes(engine.ls_svd_workspace_bytes(n, L, peek, nb), fill)
        engine.ls_svd_execute(dev(host[0]), dev(host[1]), out, n, L, peek, None, nb, stride, ostride, taps, sv, info, ws)
        torch.cuda.synchronize()
        o, t, s, i3 = out.cpu().numpy(), taps.cpu().numpy(), sv.cpu().numpy(), info.cpu().numpy()
        return dict(frames=[(o[i, :n].copy(), t[i].copy(), s[i].copy(), i3[i].copy(), untouched(o[i, n:], fill)) for i in range(nb)],
                    whole=None)

    @staticmethod
    def check(case, f, got, want):
        from conftest import rel_err
        out, taps, sv, (kept, sweeps, conv), gap = got
        w = want[f]
        assert gap, f"block {f}: out was written beyond its n elements"
        assert conv == 1 and kept == w["kept"] == case["L"] + case["peek"], f"block {f}: kept {kept} of {w['kept']}, converged {conv}"
        e = rel_err(out, w["out"])
        assert e <= 1e-4, f"block {f}: out {e:.3g}"
        assert np.abs(sv - w["sv"]).max() <= 1e-6 * w["sv"][0], f"block {f}: singular values"


LsSvd.STRADDLE = {
    "ls_svd.T = 1 (no pair)": (lambda c: c["L"] + c["peek"] == 1, {False, True}),
    "ls_svd.T = 2 (one pair)": (lambda c: c["L"] + c["peek"] == 2, {False, True}),
    "ls_svd.T odd (a bye)": (lambda c: (c["L"] + c["peek"]) % 2 == 1 and c["L"] + c["peek"] > 1, {False, True}),
    "ls_svd.LAG_GROUP": (lambda c: c["L"] + c["peek"] > LsSvd.LAG_GROUP, {False, True}),
    "ls_svd.TILE": (lambda c: c["n"] > LsSvd.TILE, {False, True}),
    "ls_svd.peek 0": (lambda c: c["peek"] == 0, {False, True}),
    "ls_svd.blocks": (lambda c: c["nblocks"], {1, 2, 3}),
    "ls_svd.stride gap": (lambda c: c["gap"] > 0 and c["nblocks"] > 1, {False, True}),
}


# ---- eca -------------------------------------------------------------------------------------------------------------------------
class Eca(Kind):
    name, header = "eca", "ECA_Filter"
    BINS = (0.0, 1.0, -1.0, 2.0, -2.0)      # Hz on a 0.5 s block, as tests/eca_oracle.py's scene
    MAX_COND = 1e5                          # the conditioning tests/test_gpu_ls_eca.py states its bars for
    CHUNK = 4096                            # ECA_MIN_CHUNK of csrc/eca.hip: samples per workgroup of the correlation

    @staticmethod
    def draw(rng):
        L, peek = pick(rng, [(1, 0), (1, 0), (2, 0), (6, 10), (16, 0), (16, 10), (23, 4)])
        return dict(kind="eca", n=pick(rng, [257, 1021, 4096, 4099, 6001]), L=L, peek=peek, nbins=pick(rng, [1, 2, 3, 4, 5, 5]),
                    reg=pick(rng, [0.0, 0.0, 1.0, 50.0]), nblocks=int(rng.integers(1, 4)), gap=pick(rng, [0, 37]),
                    seed=int(rng.integers(1 << 30)))

    @staticmethod
    def nframes(case):
        return case["nblocks"]

    @staticmethod
    def geometry(case):
        return 2.0 * case["n"], Eca.BINS[:case["nbins"]]

    @staticmethod
    def inputs(case):
        """white reference; echoes at small delays a tenth of a resolution cell off their bins, a weak far target, noise"""
        out = []
        n = case["n"]
        fs, bins = Eca.geometry(case)
        t, cell = np.arange(n, dtype=np.float64), fs / n
        for b in range(case["nblocks"]):
            rng = seeded(case, b)
            ref = cwhite(rng, n)
            srv = 0.01 * np.roll(ref, 9) * np.exp(2j * np.pi * 40.0 * cell * t / fs) + 0.001 * cwhite(rng, n)
            for d, (f, a) in enumerate(zip(bins, (1.0, 0.3, 0.2, 0.1, 0.1))):
                srv = srv + a * np.roll(ref, d % 4) * np.exp(2j * np.pi * (f + 0.1 * cell * (f != 0)) * t / fs)
            out.append((ref, srv.astype(np.complex64)))
        return out

    @staticmethod
    def expected(case):
        import eca_oracle as E
        fs, bins = Eca.geometry(case)
        out = []
        for ref, srv in inputs(case):
            o, _, (G, _, _) = E.ECA_Filter(ref, srv, case["L"], fs, bins, case["peek"], case["reg"], True, True)
            out.append(dict(out=o, cond=float(np.linalg.cond(G))))
        return out

    @staticmethod
    def conditioned(case, want):
        for w in want:
            assert w["cond"] <= Eca.MAX_COND, f"cond(G) = {w['cond']:.3g}"

    @staticmethod
    def run(case, order, fill, plain):
        import torch
        from passiveradar_amd import engine
        xs = inputs(case)
        order = list(range(case["nblocks"])) if order is None else order
        fs, bins = Eca.geometry(case)
        nb, n, L, peek, B = len(order), case["n"], case["L"], case["peek"], case["nbins"]
        stride, ostride = n + case["gap"], n + (case["gap"] and case["gap"] - 16)
        host = np.full((2, nb, stride), np.nan, np.complex64)
        for i, f in enumerate(order):
            host[0, i, :n], host[1, i, :n] = xs[f]
        out = dev_out((nb, ostride), torch.complex64, fill)
        taps, info = dev_out((nb, B, L + peek), torch.complex128, fill), dev_out((nb,), torch.int32, fill)
        ws = dev_bytes(engine.eca_workspace_bytes(n, L, peek, B, nb), fill)
        engine.eca_execute(dev(host[0]), dev(host[1]), out, n, L, peek, fs, bins, case["reg"], nb, stride, ostride, taps, info, ws)
        torch.cuda.synchronize()
        o, t, i1 = out.cpu().numpy(), taps.cpu().numpy(), info.cpu().numpy()
        return dict(frames=[(o[i, :n].copy(), t[i].copy(), i1[i].copy(), untouched(o[i, n:], fill)) for i in range(nb)], whole=None)

    @staticmethod
    def check(case, f, got, want):
        import eca_oracle as E
        from conftest import rel_err
        from passiveradar_amd.signal_utils import frequency_shift
        from test_gpu_ls_eca import solve_bar
        out, taps, info, gap = got
        w = want[f]
        assert gap, f"block {f}: out was written beyond its n elements"
        e = rel_err(out, w["out"])
        assert info == 0 and e <= 1e-4, f"block {f}: info {info}, out {e:.3g}, cond {w['cond']:.3g}"
        fs, bins = Eca.geometry(case)
        ref, srv = inputs(case)[f]          # the solve alone, on the device's own regressors (test_shapes)
        _, ets = E.ECA_Filter(ref, srv, case["L"], fs, bins, case["peek"], case["reg"], True, shift=frequency_shift)
        es = rel_err(taps, ets)
        assert es <= solve_bar(w["cond"]), f"block {f}: taps {es:.3g} on the device's regressors, bar {solve_bar(w['cond']):.3g}"


Eca.STRADDLE = {
    "eca.bins": (lambda c: c["nbins"], {1, 2, 3, 4, 5}),
    "eca.T = 1": (lambda c: c["L"] + c["peek"] == 1, {False, True}),
    "eca.reg": (lambda c: c["reg"] > 0, {False, True}),
    "eca.CHUNK": (lambda c: c["n"] > Eca.CHUNK, {False, True}),
    "eca.stride gap": (lambda c: c["gap"] > 0 and c["nblocks"] > 1, {False, True}),
}


# ---- patch -----------------------------------------------------------------------------------------------------------------------
class Patch(Kind):
    name, header = "patch", "exact cross-ambiguity patches"
    RUN = 16                                # csrc/xambg_patch.hip: samples of one float32 Horner run
    NARROW_LAGS = 32                        # up to here a workgroup takes 16 lags, above 64

    @staticmethod
    def draw(rng):
        n = pick(rng, [61, 1000, 1021, 1024, 2049, 4099])
        nlags = pick(rng, [1, 3, 16, 27, 32, 33, 64])
        npatches = pick(rng, [1, 2] if nlags > 32 else [1, 2, 3, 5, 5])      # the oracle is a matrix product per lag
        touch = [pick(rng, ["lag 0", "lag n-1", "negative", "inside"]) for _ in range(npatches)]
        lags = []
        for t in touch:
            lo = {"lag 0": -(nlags // 2), "lag n-1": n - 1 - nlags // 2, "negative": -int(rng.integers(1, n)),
                  "inside": int(rng.integers(0, n // 2))}[t]
            lags.append(int(min(max(lo, -(n - 1)), n - 1)))
        return dict(kind="patch", n=n, nlags=nlags, ndoppler=pick(rng, [1, 5, 16, 17]), step=pick(rng, [0.5, 0.25, 1.0]), lags=tuple(lags),
                    touch=tuple(touch), dopplers=tuple(float(np.round(rng.uniform(-0.4 * n, 0.4 * n), 2)) for _ in range(npatches)),
                    wrap=bool(rng.integers(2)), window=bool(rng.integers(2)), nframes=int(rng.integers(1, 3)), seed=int(rng.integers(1 << 30)))

    @staticmethod
    def nframes(case):
        return len(case["lags"])            # the patches are the batch

    @staticmethod
    def inputs(case):
        from passiveradar_amd import scene
        n = case["n"]
        pairs = [scene.make_scene(n, float(n), 16, int(case["seed"]) % 100000 + b) for b in range(case["nframes"])]
        frame = [k % case["nframes"] for k in range(len(case["lags"]))]
        return dict(ref=np.stack([p[0] for p in pairs]), srv=np.stack([p[1] for p in pairs]), frame=frame,
                    window=np.kaiser(n, 5.0).astype(np.float32) if case["window"] else None)

    @staticmethod
    def expected(case):
        import xambg_patch_oracle as PO
        x = inputs(case)
        X = PO.patches(x["ref"], x["srv"], float(case["n"]), case["lags"], case["dopplers"], case["nlags"], case["ndoppler"], case["step"],
                       x["window"], case["wrap"], x["frame"])
        scale = max(PO.bound(x["ref"][b], x["srv"][b], x["window"]) for b in range(case["nframes"]))
        return dict(X=X, scale=scale)

    @staticmethod
    def run(case, order, fill, plain):
        from passiveradar_amd.range_doppler_processing import xambg_patch
        from passiveradar_amd.target_detection import refine_peaks
        x = inputs(case)
        order = list(range(len(case["lags"]))) if order is None else order
        lags, dops = [case["lags"][k] for k in order], [case["dopplers"][k] for k in order]
        X = xambg_patch(x["ref"], x["srv"], float(case["n"]), lags, dops, case["nlags"], case["ndoppler"], case["step"], x["window"],
                        case["wrap"], [x["frame"][k] for k in order])
        pk = refine_peaks(X, lags, dops, case["step"])
        return dict(frames=[(X[i], pk[i:i + 1].copy()) for i in range(len(order))], whole=None)

    @staticmethod
    def check(case, f, got, want):
        import xambg_patch_oracle as PO
        from test_gpu_patch import BAR, assert_peaks_equal
        X, pk = got
        assert X.dtype == np.complex64 and X.shape == want["X"][f].shape
        e = float(np.abs(X - want["X"][f]).max() / want["scale"])
        assert e <= BAR, f"patch {f}: {e:.3g} of the bound"
        assert_peaks_equal(pk, PO.refine(X[None], [case["lags"][f]], [case["dopplers"][f]], case["step"]), case["step"])


Patch.STRADDLE = {
    "patch.RUN divides n": (lambda c: c["n"] % Patch.RUN == 0, {False, True}),
    "patch.NARROW_LAGS": (lambda c: c["nlags"] > Patch.NARROW_LAGS, {False, True}),
    "patch.touches": (lambda c: set(c["touch"]), {"lag 0", "lag n-1", "negative", "inside"}),
    "patch.wrap": (lambda c: c["wrap"], {False, True}),
    "patch.window": (lambda c: c["window"], {False, True}),
    "patch.patches": (lambda c: len(c["lags"]), {1, 2, 5}),
}


# ---- echo ------------------------------------------------------------------------------------------------------------------------
class Echo(Kind):
    name, header = "echo", "joint least-squares removal of strong echoes"
    RUN = 16                                # EC_RUN of csrc/echo.hip: samples that share a float64 phase seed
    MAX_ATOMS = 32                          # PRC_ECHO_MAX_ATOMS
    MAX_COND = 100.0                        # tests/test_gpu_echo.py states its bars for cond(G) < 100

    @staticmethod
    def draw(rng):
        ramp = bool(rng.integers(4))
        counts = tuple(pick(rng, [0, 1, 1, 2, 2, 5, 12, 32]) for _ in range(int(rng.integers(1, 4))))
        sizes = [4096, 4099] if max(counts) >= 12 else [1500, 2500, 3001, 4096, 4099] + ([61, 61] if max(counts) <= 2 else [])
        return dict(kind="echo", n=pick(rng, sizes),
                    counts=counts, wrap=bool(rng.integers(2)), ramp=ramp, refine=int(rng.integers(0, 3)) if ramp else 0,
                    reg=pick(rng, [0.0, 0.0, 150.0]), gap=pick(rng, [0, 37]), seed=int(rng.integers(1 << 30)))

    @staticmethod
    def nframes(case):
        return len(case["counts"])

    @staticmethod
    def inputs(case):
        """per frame: white reference, srv = k echoes (lags 3 j + 1 -- the first at lag 0 --, Dopplers spread over +-40 cells, falling
        amplitudes) + noise; the listed Dopplers are a fraction of a cell off, exactly on without the slope columns"""
        import echo_oracle as EO
        out = []
        n = case["n"]
        fs = float(n)
        for b, k in enumerate(case["counts"]):
            rng = seeded(case, b)
            ref = cwhite(rng, n)
            echoes = [((3 * j + 1) % max(n - 1, 1) if j else 0, ((17 * j + 5 * b) % 81 - 40) * min(1.0, n / 200.0) + 0.37, 1.0 / (1 + 0.3 * j))
                      for j in range(k)]
            srv = 1e-3 * cwhite(rng, n).astype(np.complex128)
            for lag, f, amp in echoes:
                srv = srv + EO.echo(ref, lag, f, fs, amp, case["wrap"])
            off = [(0.2 * (-1) ** j if case["ramp"] and case["refine"] else 0.0) for j in range(k)]
            out.append(dict(ref=ref, srv=srv.astype(np.complex64), lags=[e[0] for e in echoes], dops=[e[1] + o for e, o in zip(echoes, off)]))
        return out

    @staticmethod
    def kw(case):
        return dict(wrap=case["wrap"], ramp=case["ramp"], refine=case["refine"], reg=case["reg"])

    @staticmethod
    def expected(case):
        import echo_oracle as EO
        return [EO.cancel(x["ref"], x["srv"], float(case["n"]), x["lags"], x["dops"], return_cond=True, **Echo.kw(case)) for x in inputs(case)]

    @staticmethod
    def conditioned(case, want):
        for out, fit, info, cond in want:
            assert info == 0 and cond < Echo.MAX_COND, f"oracle info {info}, cond(G) {cond:.3g}"

    @staticmethod
    def run(case, order, fill, plain):
        from test_gpu_echo import run as echo_run
        xs = inputs(case)
        order = list(range(len(case["counts"]))) if order is None else order
        n = case["n"]
        out, fit, info, before, after = echo_run(np.stack([xs[f]["ref"] for f in order]), np.stack([xs[f]["srv"] for f in order]), float(n),
                                                 [xs[f]["lags"] for f in order], [xs[f]["dops"] for f in order],
                                                 max_atoms=max(max(case["counts"]), 1),
                                                 stride=n + case["gap"], out_stride=n + (case["gap"] and case["gap"] - 16), fill=fill,
                                                 **Echo.kw(case))
        assert np.array_equal(before, after), "the caller's atom list was written"
        return dict(frames=[(out[i].copy(), fit[i].copy(), info[i].copy()) for i in range(len(order))], whole=None)

    @staticmethod
    def check(case, f, got, want):
        from test_gpu_echo import hold
        out, fit, info = got
        x = inputs(case)[f]
        hold(f"frame {f}", out, fit, info, x["ref"], x["srv"], float(case["n"]), x["lags"], x["dops"], **Echo.kw(case))
        if not x["lags"]:
            assert np.array_equal(out.view(np.uint32), x["srv"].view(np.uint32)), f"frame {f}: no atom, yet out is not srv bit for bit"


Echo.STRADDLE = {
    "echo.atoms": (lambda c: set(c["counts"]), {0, 1, 2, Echo.MAX_ATOMS}),
    "echo.frames with different counts": (lambda c: len(set(c["counts"])) > 1, {False, True}),
    "echo.wrap": (lambda c: c["wrap"], {False, True}),
    "echo.ramp": (lambda c: c["ramp"], {False, True}),
    "echo.refine": (lambda c: c["refine"], {0, 1, 2}),
    "echo.RUN divides n": (lambda c: c["n"] % Echo.RUN == 0, {False, True}),
}


KINDS = {k.name: k for k in (Gal, Track, Strack, Persistence, Display, Welch, Preproc, LsSvd, Patch, CfarOs, Eca, Plots, Tbd, Echo)}
FUZZ_KINDS = dict(enumerate(KINDS, start=26))      # the numbers tests/fuzz_parity.py takes in PR_FUZZ_KINDS: 26 .. 39


def preload():
    """import everything the runners and the checks use, on the calling thread: a worker thread's first import of torch can
    deadlock with another worker's HIP call (the header of tests/fuzz_parity.py has the stacks)"""
    import importlib
    for m in ("torch", "conftest", "passiveradar_amd._lib", "passiveradar_amd.engine", "passiveradar_amd.scene",
              "passiveradar_amd.target_detection", "passiveradar_amd.plotting_tools", "passiveradar_amd.spectral",
              "passiveradar_amd.signal_utils", "passiveradar_amd.range_doppler_processing", "passiveradar_amd.clutter_removal",
              "cfar_os_oracle", "plots_oracle", "tbd_oracle", "tracker_oracle", "simple_tracker_oracle", "display_oracle", "psd_oracle",
              "preproc_oracle", "gal_oracle", "ls_svd_oracle", "eca_oracle", "xambg_patch_oracle", "echo_oracle", "test_gpu_cfar_os",
              "test_gpu_plots", "test_simple_tracker_host", "test_gpu_psd", "test_gpu_preproc", "test_gpu_ls_eca", "test_gpu_patch",
              "test_gpu_echo"):
        importlib.import_module(m)


def fuzz_one(number, rng, plain=False):
    """one random case of fuzz kind ``number`` (26 .. 39) for tests/fuzz_parity.py: (kind name, 0.0 or 1.0, what to print);
    ``plain``: several caller threads, so the process-wide switches stay as they are"""
    kind = KINDS[FUZZ_KINDS[int(number)]]
    while True:                             # a random draw on which the oracle alone is not to be trusted is drawn again, not run
        case = kind.draw(rng)
        try:
            kind.conditioned(case, expected(case))
            break
        except AssertionError:
            _EXPECTED.pop(repr(case), None)
    try:
        check(case, run(case, plain=plain))
        return "sweep_" + kind.name, 0.0, case
    except AssertionError as e:
        return "sweep_" + kind.name, 1.0, str(e)[-600:]
    finally:
        _EXPECTED.pop(repr(case), None)
        _INPUTS.pop(repr(case), None)
