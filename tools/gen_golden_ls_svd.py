"""Writes tests/golden/ls_svd_*.npz from the reference's own LS_Filter_SVD (passiveRadar/clutter_removal.py:58-107).  Run
where the reference checkout exists (CPU only):

    python tools/gen_golden_ls_svd.py [--reference PATH]

Each file holds the inputs (ref, srv), the arguments (filterLen, peek), the reference's (out, taps) in complex64, the NumPy
and SciPy versions that produced them, and the reference's own distance to the float64 restatement (tests/ls_svd_oracle.py
at its default cut): dist_out and dist_taps, max |difference| / max |restatement| -- the float32 floor of the reference
itself, which the host test holds the restatement to (2x) and which leaves the 1e-4 parity bar of the GPU test its room.

The cases are the inputs on which the reference is a usable oracle: white references, a mildly coloured one (AR(2), pole
radius 0.9, cond(A) ~ 50), an exactly periodic one (rank 8 of 26: the reference's float32 SVD returns exact zeros for the
null directions and drops them), that plus 1e-2 of white noise (cond ~ 300) and a silent one.  AR(2) at radius 0.99 and
band-limited references get no golden: the reference's own error there is 1e-4 and 26."""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden")
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

# name: (input, n, filterLen, peek, seed)
CASES = {
    "ls_svd_white": ("white", 4099, 16, 10, 6100),
    "ls_svd_white_peek0": ("white", 1021, 37, 0, 6200),
    "ls_svd_white_t74": ("white", 4099, 64, 10, 6300),
    "ls_svd_ar2": ("ar2", 4099, 16, 10, 6400),
    "ls_svd_periodic": ("periodic", 4096, 16, 10, 6500),
    "ls_svd_periodic_noise": ("periodic_noise", 4096, 16, 10, 6600),
    "ls_svd_zero_ref": ("zero", 1024, 16, 10, 6700),
}


def cwhite(rng, n):
    return ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2.0)).astype(np.complex64)


def make_reference_channel(kind, n, rng):
    if kind == "white":
        return cwhite(rng, n)
    if kind == "ar2":                                   # poles at 0.9 exp(+-0.3j)
        x = cwhite(rng, n + 500).astype(np.complex128)
        y = np.zeros_like(x)
        a1, a2 = 2 * 0.9 * np.cos(0.3), -0.81
        for i in range(2, x.shape[0]):
            y[i] = x[i] + a1 * y[i - 1] + a2 * y[i - 2]
        y = y[500:]
        return (y / np.abs(y).std()).astype(np.complex64)
    if kind in ("periodic", "periodic_noise"):
        ref = np.tile(cwhite(rng, 8), n // 8)
        return ref if kind == "periodic" else (ref + 1e-2 * cwhite(rng, n)).astype(np.complex64)
    return np.zeros(n, np.complex64)


def make_inputs(kind, n, filterLen, peek, seed):
    """reference channel of the named kind; surveillance = a decaying filter of T taps applied to its circular shifts, plus
    white noise at 0.05"""
    rng = np.random.default_rng(seed)
    ref = make_reference_channel(kind, n, rng)
    T = filterLen + peek
    h0 = cwhite(rng, T) * np.exp(-np.arange(T) / 6.0)
    clutter = sum(h0[k] * np.roll(ref.astype(np.complex128), k - peek) for k in range(T))
    return ref, (clutter + 0.05 * cwhite(rng, n)).astype(np.complex64)


def rel(a, b):
    s = float(np.abs(b).max())
    return float(np.abs(a - b).max()) / (s if s > 0 else 1.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("PASSIVERADAR_REFERENCE"), required="PASSIVERADAR_REFERENCE" not in os.environ,
                    help="checkout of the reference (Max-Manning/passiveRadar)")
    ap.add_argument("--only", default=None, help="comma-separated case names")
    args = ap.parse_args()
    sys.path.insert(0, args.reference)
    import scipy
    from passiveRadar.clutter_removal import LS_Filter_SVD as ref_svd
    from ls_svd_oracle import ls_filter_svd
    names = args.only.split(",") if args.only else list(CASES)
    for name in names:
        kind, n, L, peek, seed = CASES[name]
        ref, srv = make_inputs(kind, n, L, peek, seed)
        with np.errstate(divide="ignore"):                 # 1 / S of the singular values the reference then drops
            out, taps = ref_svd(ref, srv, L, peek, return_filter=True)
        info = {}
        eo, et = ls_filter_svd(ref, srv, L, peek, None, info)
        sv = info["sv"]
        d_out, d_taps = rel(out, eo), rel(taps, et)
        cond = sv[0] / sv[info["kept"] - 1] if info["kept"] else 0.0
        print(f"{name}: n {n} T {L + peek} kept {info['kept']} cond (kept) {cond:.3g}  reference against the restatement: "
              f"out {d_out:.1e} taps {d_taps:.1e}  ({out.dtype}, {taps.dtype})", flush=True)
        np.savez_compressed(os.path.join(OUT, name + ".npz"), ref=ref, srv=srv, out=out, taps=taps,
                            filterLen=np.int64(L), peek=np.int64(peek), dist_out=np.float64(d_out),
                            dist_taps=np.float64(d_taps), numpy_version=np.str_(np.__version__),
                            scipy_version=np.str_(scipy.__version__))


if __name__ == "__main__":
    main()
