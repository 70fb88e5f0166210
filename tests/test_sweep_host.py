"""The seeded sweep of tests/sweep_cases.py, as far as it runs without a GPU: the case lists are reproducible and cross every
named switch point, every case has an oracle result and is one on which that oracle can be trusted (none is left out), the
kinds are the entry-point families of include/prcore.h added after kind 25 of tests/fuzz_parity.py, and for the kinds whose
output is exact the oracle is held to an independent brute-force statement on three tiny cases of the sweep's own inputs."""
import math
import os
import re

import numpy as np
import pytest

import sweep_cases as SC
from conftest import REPO

KIND_NAMES = list(SC.KINDS)


def test_fourteen_kinds_cover_the_header_sections_added_after_kind_25():
    """every section of include/prcore.h is either one the fuzzer's kinds 0 - 25 already reach or begins as exactly one kind's
    ``header`` does: an entry-point family added without a kind shows here"""
    old = ("library / device", "cross-ambiguity surface", "block least-squares clutter cancellers", "NLMS_filter",
           "helpers that sit on the path", "front end", "CFAR_2D", "channel offset estimation", "frame gather over xGMI")
    with open(os.path.join(REPO, "include", "prcore.h")) as fh:
        titles = [line[8:].strip() for line in fh if line.startswith("/* ---- ")]
    assert len(titles) >= 23
    seen = []
    for t in titles:
        if t.startswith(old):
            continue
        owners = [k.name for k in SC.KINDS.values() if t.startswith(k.header)]
        assert len(owners) == 1, f"section {t!r} of include/prcore.h belongs to the kinds {owners}"
        seen += owners
    assert sorted(seen) == sorted(KIND_NAMES) and len(KIND_NAMES) == 14
    assert list(SC.FUZZ_KINDS) == list(range(26, 40)) and list(SC.FUZZ_KINDS.values()) == KIND_NAMES
    for k in SC.KINDS.values():                               # the module docstring names each section against its kind
        assert f"-> {k.name}" in SC.__doc__, k.name


def test_descriptors_are_reproducible_and_independent_of_other_kinds():
    first = {k: [repr(c) for c in SC.cases(k)] for k in KIND_NAMES}
    for k in reversed(KIND_NAMES):                            # drawn again, in another order
        again = SC.cases(k)
        assert len(again) == SC.NCASES == 24 and [repr(c) for c in again] == first[k], k
        assert all(c["kind"] == k and isinstance(c["seed"], int) for c in again)
        assert [repr(c) for c in SC.cases(k, seed=SC.SEED + 1)] != first[k]
    for k in KIND_NAMES:                                      # a descriptor is sizes, options and a seed: eval(repr) is the case
        for c in SC.cases(k):
            assert eval(repr(c)) == c


def test_named_constants_are_the_librarys():
    """the switch points that the Python layer mirrors, and those that live only in a kernel's source"""
    from passiveradar_amd import _lib
    assert SC.Plots.LDS_CELLS == _lib.PLOTS_LDS_CELLS and SC.Tbd.FRAMES == _lib.TBD_FRAMES
    assert SC.Persistence.TERMS_PER_LAUNCH == _lib.PERSISTENCE_TERMS_PER_LAUNCH and SC.Preproc.TILE_MAX_Q == _lib.FIRDEC_TILE_MAX_Q
    assert SC.Echo.MAX_ATOMS == _lib.ECHO_MAX_ATOMS
    src = {}

    def has(name, pattern):
        if name not in src:
            with open(os.path.join(REPO, "passiveradar_amd", "csrc", name)) as fh:
                src[name] = fh.read()
        assert re.search(pattern, src[name]), (name, pattern)
    has("cfar_os.hip", rf"#define CO_TX {SC.CfarOs.TILE_COLS}\b")
    has("cfar_os.hip", rf"#define CO_TY {SC.CfarOs.TILE_ROWS}\b")
    has("track.hip", rf"constexpr int LDS_CAP = {SC.Track.LDS_CAP};")
    has("gal.hip", rf"#define GAL_FAST_MAX {SC.Gal.FAST_MAX}\b")
    has("gal.hip", r"tpls\[\] = \{1, 2, 3, 4, 5, 6, 7, 8, 10, 12,")
    has("gal.hip", rf"lattice_len <= {SC.Gal.ROW_FORM_LATTICE};")
    has("ls_svd.hip", rf"#define SVD_TILE {SC.LsSvd.TILE}\b")
    has("eca.hip", rf"#define ECA_MIN_CHUNK {SC.Eca.CHUNK}\b")
    has("echo.hip", rf"constexpr int EC_RUN = {SC.Echo.RUN};")
    has("preproc.hip", r"constexpr int FD_T = 64;")
    has("preproc.hip", r"constexpr int FD_R = 4;")
    assert SC.Preproc.TILE_OUTPUTS == 64 * 4


def test_every_switch_point_is_crossed():
    """for every named switch point the seeded list of its kind holds at least one case on each side"""
    names, missing = [], []
    for k in KIND_NAMES:
        cases = SC.cases(k)
        assert SC.KINDS[k].STRADDLE, k
        for name, (side, need) in SC.KINDS[k].STRADDLE.items():
            assert name.startswith(k + "."), name
            seen = set()
            for c in cases:
                v = side(c)
                seen |= set(v) if isinstance(v, (set, frozenset, list)) else {v}
            names.append(name)
            if not set(need) <= seen:
                missing.append((name, sorted(map(repr, set(need) - seen))))
    print(f"{len(names)} switch points: " + "; ".join(names))
    assert not missing, f"the seeded lists no longer cross: {missing}"
    assert len(names) == len(set(names)) >= 90


@pytest.mark.parametrize("kind", KIND_NAMES)
def test_every_case_has_a_trustworthy_oracle_result(kind):
    """expected(case) runs for all 24 cases and the conditioning checks hold for every one: zero cases are left out"""
    k = SC.KINDS[kind]
    cases = SC.cases(kind)
    for c in cases:
        want = SC.expected(c)
        try:
            k.conditioned(c, want)
        except AssertionError as e:
            raise AssertionError(f"{c!r}: {e}") from e
        n = k.nframes(c)
        assert n >= 1 and all(len(o) >= 1 and set(o) <= set(range(n)) for o in k.orders(c))
    assert len(cases) == 24


# ---- second witnesses for the kinds with exact output ---------------------------------------------------------------------------
def tiny(kind, size, ok=lambda c: True):
    """the three smallest cases of a kind's seeded list"""
    cs = sorted((c for c in SC.cases(kind) if ok(c)), key=size)[:3]
    assert len(cs) == 3
    return cs


def brute_plots(stat, thresh, ext, weight, connectivity, range_guard, doppler_guard):
    """prc_plots of include/prcore.h with union-find labelling and exactly rounded sums (math.fsum): list of dicts in output order"""
    H, W = stat.shape
    det = np.zeros((H, W), bool)
    for h in range(H):
        for w in range(W):
            zone = w < range_guard or w >= W - range_guard or (H // 2 - doppler_guard <= H - 1 - h < H // 2 + doppler_guard)
            det[h, w] = bool(stat[h, w] > np.float32(thresh)) and not zone
    parent = list(range(H * W))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i
    steps = [(0, 1), (1, 0)] + ([(1, 1), (1, -1)] if connectivity == 8 else [])
    for h in range(H):
        for w in range(W):
            for dh, dw in steps:
                y, x = h + dh, w + dw
                if det[h, w] and 0 <= y < H and 0 <= x < W and det[y, x]:
                    parent[find(h * W + w)] = find(y * W + x)
    comps = {}
    for i in range(H * W):
        if det[i // W, i % W]:
            comps.setdefault(find(i), []).append(i)

    def g(i):
        if weight is None:
            return float(stat.flat[i])
        v = weight.flat[i]
        if np.iscomplexobj(weight):
            re, im = float(v.real), float(v.imag)
            return float(np.float32(math.sqrt(re * re + im * im)))
        return float(v)
    D, R = float(ext[0]), float(ext[1])
    rows = []
    for cells in comps.values():
        peak = min(cells, key=lambda i: (-float(stat.flat[i]), i))
        M = math.fsum(g(i) for i in cells)
        hbar = math.fsum(g(i) * (i // W) for i in cells) / M
        wbar = math.fsum(g(i) * (i % W) for i in cells) / M
        hp, wp = divmod(peak, W)
        rows.append(dict(index=wp * H + (H - 1 - hp), strength=float(stat.flat[peak]), peak=peak, ncells=len(cells), mass=M, hbar=hbar,
                         wbar=wbar, range=wbar * ((0.0 - R) / (W - 1)) + R, doppler=((H - 1) - hbar) * (2.0 * D / (H - 1)) - D,
                         h0=min(i // W for i in cells), h1=max(i // W for i in cells), w0=min(i % W for i in cells),
                         w1=max(i % W for i in cells)))
    rows.sort(key=lambda r: (-r["strength"], -r["index"]))
    return rows, int(det.sum())


def test_plots_oracle_against_union_find_and_exact_sums():
    from test_gpu_plots import EXT
    for c in tiny("plots", lambda c: c["H"] * c["W"] * c["nframes"]):
        want = SC.expected(c)["frames"]
        for (stat, weight), w in zip(SC.inputs(c), want):
            rows, ncells = brute_plots(stat, SC.Plots.thresh(c), EXT, weight, c["connectivity"], *c["guards"])
            assert ncells == w["ncells_total"] and len(rows) == w["count"], c
            for name in ("index", "peak", "ncells", "h0", "h1", "w0", "w1", "strength"):
                assert [r[name] for r in rows] == w[name].tolist(), (c, name)
            for name, span in (("mass", None), ("hbar", c["H"]), ("wbar", c["W"]), ("range", EXT[1]), ("doppler", EXT[0])):
                a, b = np.array([r[name] for r in rows]), w[name]
                assert np.all(np.abs(a - b) <= 1e-12 * (np.abs(b) if span is None else span)), (c, name)


def brute_tbd(stat, qd, qr, alpha, clip, range_guard, doppler_guard, shifts, prev):
    """prc_tbd of include/prcore.h cell by cell in Python, float32 scalars"""
    N, H, W = stat.shape
    s = [0] * H if shifts is None else [int(v) for v in shifts]
    score, back = np.empty((N, H, W), np.float32), np.empty((N, H, W), np.uint8)
    last = None if prev is None else prev
    a = np.float32(alpha)
    with np.errstate(all="ignore"):
        for k in range(N):
            cur = np.empty((H, W), np.float32)
            for h in range(H):
                for w in range(W):
                    z = stat[k, h, w]
                    if w < range_guard or w >= W - range_guard or (H // 2 - doppler_guard <= H - 1 - h < H // 2 + doppler_guard):
                        z = np.float32(0.0)
                    elif z > np.float32(clip):
                        z = np.float32(clip)
                    best, code, c = np.float32(-np.inf), 255, -1
                    for dh in range(-qd, qd + 1):
                        for dw in range(-qr, qr + 1):
                            c += 1
                            hp = h + dh
                            if last is None or not 0 <= hp < H:
                                continue
                            wp = w - s[hp] + dw
                            if 0 <= wp < W and last[hp, wp] > best:
                                best, code = last[hp, wp], c
                    m = np.float32(0.0) if code == 255 else best
                    cur[h, w] = np.float32(z + np.float32(a * m))
                    back[k, h, w] = code
            score[k] = last = cur
    return score, back


def test_tbd_oracle_against_a_cell_by_cell_statement():
    import tbd_oracle as TO
    codes = lambda c: (2 * c["reach"][0] + 1) * (2 * c["reach"][1] + 1)      # noqa: E731
    for c in tiny("tbd", lambda c: c["H"] * c["W"] * c["nframes"] * codes(c)):
        x, want = SC.inputs(c), SC.expected(c)
        score, back = brute_tbd(x["stat"], c["reach"][0], c["reach"][1], c["alpha"], np.inf if c["clip"] is None else c["clip"],
                                c["guards"][0], c["guards"][1], x["shifts"], x["prev"])
        assert TO.same_bits(score, want["score"]) and np.array_equal(back, want["back"]), c


def brute_measure(frame, ext, p):
    """get_measurements with NumPy's own percentile and linspace and Python's sort"""
    H, W = frame.shape
    v = frame.astype(np.float64)
    mean = np.abs(v).sum() / v.size
    s = np.fliplr(v.T) / mean
    s[:8, :] = 0
    s[-8:, :] = 0
    s[:, H // 2 - 4:H // 2 + 4] = 0
    thr = np.percentile(s, p)
    flat = s.ravel()
    idx = sorted((i for i in range(flat.size) if flat[i] >= thr), key=lambda i: (-flat[i], -i))
    rpts, dpts = np.linspace(ext[1], 0, W), np.linspace(-ext[0], ext[0], H)
    return idx, [rpts[i // H] for i in idx], [dpts[i % H] for i in idx], [flat[i] for i in idx]


def test_track_oracle_against_numpys_percentile_and_a_plain_sort():
    for c in tiny("track", lambda c: c["H"] * c["W"] * c["nframes"]):
        for x, w in zip(SC.inputs(c), SC.expected(c)["frames"]):
            idx, rng_, dop, strength = brute_measure(x, SC.Track.EXT, c["percentile"])
            assert len(idx) == w["count"] and idx == w["idx"].tolist(), c
            assert rng_ == w["range"].tolist() and dop == w["doppler"].tolist() and strength == w["strength"].tolist(), c


def test_display_limits_oracle_against_numpys_percentile():
    for c in tiny("display", lambda c: c["shape"][0] * c["shape"][1] * c["nframes"], lambda c: c["shape"] != (1, 1)):
        for f, (lim, _) in zip(SC.inputs(c)["frames"], SC.expected(c)):
            with np.errstate(invalid="ignore", over="ignore"):
                flat = f.astype(np.float64).flatten()
                want = np.array([np.percentile(flat, c["p"][0]), c["hi_scale"] * np.percentile(flat, c["p"][1])])
            assert np.array_equal(lim, want, equal_nan=True), (c, lim, want)
