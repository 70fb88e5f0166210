"""Writes tests/golden/gal_*.npz from the reference's own GAL_JPE (passiveRadar/clutter_removal.py:251-365).  Run where the
reference checkout exists (CPU only):

    python tools/gen_golden_gal.py [--reference PATH]

Each file holds the inputs (ref, srv), the arguments (L, D, peek, mu1, mu2) and the reference's (out, k, h).  The cases
cover white, AR(2) and FM illuminators (passiveradar_amd/scene.py), L = 1, L < D and L = D, D in {8, 64, 100, 1034} and one
D > 2048 at small n, peek 0 and 10, mu1 capped (mu1 = 1e-2 > 5e-3 at the first step) and never capped, N <= peek + 1 (all
zeros) and one complex128-input case (the reference then carries h and e in complex128; the drop-in casts to complex64).

For every case it prints the restatement (tests/gal_oracle.py) in complex64 against the reference -- the host test holds
that to 2e-6 -- and the complex128 restatement against the reference: the float32 floor of the reference itself.
"""
import argparse
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden")
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

FS, RB = 262144.0, 64

# name: (illuminator, n, L, D, peek, mu1, mu2, seed, input dtype)
CASES = {
    "gal_white_L8_D64": ("white", 4096, 8, 64, 10, 1e-3, 1e-2, 7100, np.complex64),
    "gal_ar2_L8_D100_p0": ("ar2", 4096, 8, 100, 0, 1e-3, 1e-2, 7200, np.complex64),
    "gal_fm_L4_D64_cap": ("fm", 4096, 4, 64, 10, 1e-2, 1e-2, 7300, np.complex64),
    "gal_fm_L1_D8": ("fm", 2048, 1, 8, 10, 1e-3, 1e-2, 7400, np.complex64),
    "gal_ar2_L8_D8_p0": ("ar2", 4096, 8, 8, 0, 1e-3, 1e-2, 7500, np.complex64),
    "gal_white_L32_D1034": ("white", 1536, 32, 1034, 10, 1e-3, 1e-2, 7600, np.complex64),
    "gal_fm_L1034_D1034": ("fm", 400, 1034, 1034, 10, 1e-3, 1e-2, 7700, np.complex64),
    "gal_white_L16_D2100": ("white", 300, 16, 2100, 10, 1e-3, 1e-2, 7800, np.complex64),
    "gal_white_short_n11": ("white", 11, 4, 8, 10, 1e-3, 1e-2, 7900, np.complex64),
    "gal_white_short_n5": ("white", 5, 1, 4, 10, 1e-3, 1e-2, 7910, np.complex64),
    "gal_ar2_L8_D64_c128": ("ar2", 4096, 8, 64, 10, 1e-3, 1e-2, 8000, np.complex128),
}


def make_inputs(kind, n, seed, dtype):
    from passiveradar_amd import scene
    m = max(n, 64)
    if kind == "white":
        ref, srv = scene.make_scene(m, FS, RB, seed)
    elif kind == "ar2":
        ref, srv = scene.make_ar2_scene(m, FS, RB, seed)
    else:
        ref, srv = scene.make_fm_scene(m, FS, RB, seed)
    return ref[:n].astype(dtype), srv[:n].astype(dtype)


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
    from passiveRadar.clutter_removal import GAL_JPE as ref_gal
    from gal_oracle import gal_jpe
    names = args.only.split(",") if args.only else list(CASES)
    for name in names:
        kind, n, L, D, peek, mu1, mu2, seed, dt = CASES[name]
        ref, srv = make_inputs(kind, n, seed, dt)
        t0 = time.perf_counter()
        out, k, h = ref_gal(ref, srv, L, D, mu1, mu2, peek=peek, return_filter=True)
        secs = time.perf_counter() - t0
        st = {}
        o64, k64, h64 = gal_jpe(ref, srv, L, D, mu1, mu2, peek, np.complex64, True, st)
        o128, k128, h128 = gal_jpe(ref.astype(np.complex128), srv.astype(np.complex128), L, D, mu1, mu2, peek,
                                   np.complex128, True)
        line = (f"{name}: n {n} L {L} D {D} peek {peek} mu1 {mu1:g} caps {st['caps']}  ref {secs:.2f} s "
                f"({secs / max(n - peek - 1, 1) * 1e6:.0f} us/sample)  c64 restatement out {rel(o64, out):.1e} "
                f"k {rel(k64, k):.1e} h {rel(h64, h):.1e}  c128 floor out {rel(o128, out):.1e} k {rel(k128, k):.1e} "
                f"h {rel(h128, h):.1e}")
        if dt == np.complex128:
            oc, kc, hc = gal_jpe(ref.astype(np.complex64), srv.astype(np.complex64), L, D, mu1, mu2, peek, np.complex64, True)
            line += f"  complex64 cast: out {rel(oc, out):.1e} k {rel(kc, k):.1e} h {rel(hc, h):.1e}"
        print(line, flush=True)
        np.savez_compressed(os.path.join(OUT, name + ".npz"), ref=ref, srv=srv, out=out, k=k, h=h,
                            L=np.int64(L), D=np.int64(D), peek=np.int64(peek), mu1=np.float64(mu1), mu2=np.float64(mu2),
                            ref_seconds=np.float64(secs))


if __name__ == "__main__":
    main()
