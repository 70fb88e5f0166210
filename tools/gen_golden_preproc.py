"""Writes tests/golden/preproc_*.npz from the reference's own signal_utils (decimate, channel_preprocessing, shift,
offset_compensation, normalize).  Run where the reference checkout exists:

    python tools/gen_golden_preproc.py [--reference PATH]

The inputs are the seeded arrays of tests/preproc_oracle.py (the tests regenerate them); the files hold the reference's
outputs, and for the two large ones a part of the output plus checksums:

preproc_decimate.npz   y_<n>_<q> for DECIMATE_CASES, cols (300, 3) at q = 5, dt_<dtype> for DECIMATE_DTYPES
preproc_channel.npz    y_<name> for CHANNEL_CASES; long_tail = the last 300 outputs of 2^24 + 70 000 int8 samples at dec 10,
                       long_raw = the checksum of that recording
preproc_misc.npz       shift_<input>_<k>, off_<d> = (offset, checksum of the result, is-x2-itself), norm_<dtype>_<shape>
                       (every 97th value of the largest)
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden")
sys.path.insert(0, os.path.join(REPO, "tests"))
import preproc_oracle as O  # noqa: E402


def peak_err(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(b).max(), 1e-300))


def save(name, payload):
    fn = os.path.join(OUT, name)
    np.savez_compressed(fn, **payload)
    print(name, len(payload), "arrays,", os.path.getsize(fn), "bytes")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("PASSIVERADAR_REFERENCE"),
                    required="PASSIVERADAR_REFERENCE" not in os.environ,
                    help="checkout of the reference (Max-Manning/passiveRadar)")
    args = ap.parse_args()
    sys.path.insert(0, args.reference)
    from passiveRadar import signal_utils as ref

    worst = 0.0
    g = {}
    for n, q in O.DECIMATE_CASES:
        x = O.decimate_input(n, q)
        y = ref.decimate(x, q)
        assert y.dtype == np.complex64 and y.shape == (O.out_len(n, q),)
        worst = max(worst, peak_err(O.decimate(x, q), y))
        g[f"y_{n}_{q}"] = y
    x = O.decimate_input(300, 5, 3)
    g["cols"] = ref.decimate(x, 5)
    worst = max(worst, peak_err(O.decimate(x, 5), g["cols"]))
    for name in O.DECIMATE_DTYPES:
        x = O.dtype_input(name)
        y = ref.decimate(x, 5)
        assert y.dtype == O.result_dtype(x.dtype), (name, y.dtype)
        worst = max(worst, peak_err(O.decimate(x, 5), y))
        g[f"dt_{name}"] = y
    save("preproc_decimate.npz", g)
    print("decimate: restatement against the reference, worst", worst)

    g, worst = {}, 0.0
    for name, (dtype, nscalars, dec, fc, Fs) in O.CHANNEL_CASES.items():
        raw = O.channel_input(name)
        y = ref.channel_preprocessing(raw, dec, fc, Fs)
        assert y.dtype == np.complex64 and y.shape == (O.out_len(nscalars // 2, dec),)
        worst = max(worst, peak_err(O.channel_preprocessing(raw, dec, fc, Fs), y))
        g[f"y_{name}"] = y
    raw = O.long_input()
    y = ref.channel_preprocessing(raw, 10, 1e5, 2.4e6)
    g["long_tail"] = y[-O.LONG_KEEP:]
    g["long_peak"] = np.array(np.abs(y).max())
    g["long_raw"] = O.checksum(raw)
    # the restatement on the samples the tail reaches (the rotation needs their absolute indices)
    m = y.shape[0]
    lo = (m - O.LONG_KEEP) * 10 - 100
    z = O.deinterleave(raw[2 * lo:]) * O.rotation(O.LONG_SAMPLES - lo, 1e5, 2.4e6, start=lo)
    tail = O.fir_decimate(z.astype(np.complex64), 10)[10:]
    e = float(np.abs(tail - g["long_tail"]).max() / g["long_peak"])
    print("channel_preprocessing: restatement against the reference, worst", worst, "long tail", e)
    save("preproc_channel.npz", g)

    g = {}
    for name, x in O.shift_inputs().items():
        for k in O.SHIFTS:
            g[f"shift_{name}_{k}"] = ref.shift(x, k)
            assert np.array_equal(g[f"shift_{name}_{k}"], O.shift(x, k))
    x1 = O.offset_input()
    for d in O.OFFSETS:
        x2 = ref.shift(x1, d)
        os_ = ref.find_channel_offset(x1[:20000], x2[:20000], 4, 200)
        out = ref.offset_compensation(x1, x2, 20000, 4, 200)
        assert os_ == -d and np.array_equal(out, O.shift(x2, os_))
        g[f"off_{d}"] = np.concatenate(([os_, int(out is x2)], O.checksum(out.view(np.float32).view(np.int8))))
    for shape in O.NORMALIZE_SHAPES:
        for dtype in ("float32", "complex64"):
            x = O.normalize_input(shape, dtype)
            y = ref.normalize(x)
            assert y.dtype == np.dtype(dtype) and y.shape == shape
            e = peak_err(O.normalize(x), y)
            assert e < 2e-6, e
            tag = "x".join(map(str, shape))
            g[f"norm_{dtype}_{tag}"] = y if y.size < 1000 else y.reshape(-1)[::O.NORMALIZE_STRIDE]
    save("preproc_misc.npz", g)


if __name__ == "__main__":
    main()
