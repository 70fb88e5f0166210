"""Every shipped form of the two register / LDS transforms on its own, against float64.

The one-wavefront 1024-point FFT (passiveradar_amd/csrc/fft_wave.h, packed twin fft_wave_pk.h) and the four-wavefront
4096-point FFT (fft_team.h) run here through test-only probe libraries (tests/csrc), one per set of FT_* defines that
passiveradar_amd/csrc/Makefile ships (tests/test_fft_probe_host.py keeps that list complete).  The probes run on the
twiddle tables libprcore itself uploads.  Checked per form:
  a/b  every impulse, forward and through the inverse: each output is one product of rounded unit-modulus factors, so
       every twiddle entry and every index is pinned one by one (bar: 1.3e-6 absolute, derivation at IMPULSE_BAR)
  c    Gaussian noise against numpy.fft on complex128, with scipy.fft on the same complex64 input as the yardstick:
       relative rms error and max / peak error at most 3 x the yardstick's
  d    bit identity where the project claims it (packed = scalar; FT_TW2_REGS = 14 = 16; FT_NBUF = 1 = 2)
  e    zero-tail forms (NZ = 8, 12) equal the full form    f  PRESCALED inverse    g  repeatability of the schedules
and the packed primitives of fft_pk.h against the scalar forms they replace, bit for bit.

Measured on an MI355X (the tests print every figure, `pytest -s`, lines FIGURES_MEASURED; yardstick: scipy.fft, complex64):

  form                                        impulse fwd / inv     forward      inverse      inv of fwd   schedule
  wave 1024, scalar = FT_PK (same bits)       2.14e-7 / 1.96e-7     0.97 / 0.94  0.96 / 1.03  0.99 / 1.01  1.00 / 1.09
  team 4096, scalar = FT_PK, FT_NBUF 1 = 2,
    FT_TW2_REGS 14 = 16 (same bits)           2.67e-7 / 2.82e-7     0.97 / 1.03  0.97 / 0.92  1.01 / 0.96  1.02 / 1.01 (*)
  team 4096, FT_PK FT_NBUF=2 TW2_FACTORED     2.84e-7 / 2.82e-7     1.00 / 1.03  0.99 / 0.90  1.04 / 1.00  1.05 / 1.07
  impulse: largest absolute error over every impulse and every instantiation (bar 1.3e-6); the other columns: relative rms
  error / (max error / peak) as multiples of the yardstick's (bar 3), which itself measures 1.1e-7 (1024) and 1.3e-7 (4096)
  rms for one transform, 1.6e-7 / 1.8e-7 for the round trip, 2.1e-7 / 2.3e-7 for the schedule.
  (*) the fused LS pass's order fwd<1>, inv<0> with one inverse per piece: 1.02 / 1.11
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")

# An impulse meets only zeros in every addition, so an output is a product of at most six rounded unit-modulus factors
# (one dft16 constant per radix-16 pass, TW1, TW2, the second factor of FT_TW2_FACTORED): six factors each within
# sqrt(2) 2^-25 of the point of the unit circle they stand for, and six complex products each within sqrt(2) 2^-23:
# 6 sqrt(2) (2^-25 + 2^-23) = 1.26e-6.  A wrong table index costs at least 2 pi / 4096 = 1.5e-3.
IMPULSE_BAR = 1.3e-6
YARDSTICK_FACTOR = 3.0

# (id, library) -- the ids name the flag set
TEAM_FORMS = [("team_scalar_nbuf2", "libfftprobe.so"), ("team_scalar_nbuf1", "libfftprobe1.so"),
              ("team_pk_nbuf2", "libfftprobe_pk2.so"), ("team_pk_nbuf2_tw2factored", "libfftprobe_pk2f.so"),
              ("team_pk_nbuf1_tw2regs14", "libfftprobe_pk1r14.so"), ("team_pk_nbuf1", "libfftprobe_pk1.so")]
WAVE_FORMS = [("wave_scalar", "libfftprobe_wave.so"), ("wave_pk", "libfftprobe_wave_pk.so")]
FORMS = dict(TEAM_FORMS + WAVE_FORMS)
TEAM_IDS = [f for f, _ in TEAM_FORMS]
WAVE_IDS = [f for f, _ in WAVE_FORMS]
# probe_flags of fft_probe.hip: NBUF | PK << 4 | FACTORED << 5 | TW2_REGS << 8
TEAM_FLAGS = {"team_scalar_nbuf2": 2 | 16 << 8, "team_scalar_nbuf1": 1 | 16 << 8, "team_pk_nbuf2": 2 | 1 << 4 | 16 << 8,
              "team_pk_nbuf2_tw2factored": 2 | 1 << 4 | 1 << 5 | 16 << 8, "team_pk_nbuf1_tw2regs14": 1 | 1 << 4 | 14 << 8,
              "team_pk_nbuf1": 1 | 1 << 4 | 16 << 8}

# modes of the probes (tests/csrc/fft_probe.hip, fft_probe_wave.hip): name -> (mode, zero tail NZ or None)
TEAM_FWD = {"ft4096_fwd_0": (0, 16), "ft4096_fwd_1": (3, 16), "ft4096_fwd_0_nz12": (4, 12), "ft4096_fwd_0_nz8": (5, 8),
            "ft4096_fwd_1_nz12": (6, 12), "ft4096_fwd_1_nz8": (7, 8)}
TEAM_INV = {"ft4096_inv_0": 8, "ft4096_inv_1": 9}
TEAM_ROUNDTRIP = 1
TEAM_SCHED = {"sched_fwd0_fwd1_inv1": 2, "sched_caf_fwd0_fwd1_inv0_sync": 10, "sched_ls_cached_fwd1_inv0": 11}
WAVE_FWD = {"fft1024_fwd_16": (0, 16), "fft1024_fwd_12": (1, 12), "fft1024_fwd_8": (2, 8)}
WAVE_INV = {"fft1024_inv": 3, "fft1024_inv_prescaled": 4}
WAVE_ROUNDTRIP = 5
WAVE_SCHED = {"sched_fwd_fwd_inv": 6}

NOISE = 256              # transforms of noise per form
TEAM_COPIES = 5          # 1280 workgroups: more than the 1024 the chip holds at once (256 CUs x 4 of 37 KB LDS at most)
WAVE_COPIES = 16         # 4096 transforms = 1024 workgroups of four waves: more than the 768 that fit (44 KB LDS each)


def _is_team(form):
    return form.startswith("team")


def _P(form):
    return 4096 if _is_team(form) else 1024


def _bins(P):
    """frequency bin of every element of the frequency layout (fft_team.h:12, fft_wave.h:11)"""
    if P == 4096:
        t = np.arange(256)[:, None]
        r = np.arange(16)[None, :]
        return ((t >> 4) + 16 * (t & 15) + 256 * r).reshape(-1)
    lane = np.arange(64)[:, None]
    r = np.arange(16)[None, :]
    jb = lane & 3
    bitrev2 = ((jb & 1) << 1) | (jb >> 1)
    return ((lane >> 2) + 16 * r + 256 * bitrev2).reshape(-1)


@pytest.fixture(scope="module")
def run(gpu_ready):
    """run(form, mode, x, y=None) -> output of the probe on x (and y, where the mode reads two inputs)"""
    if any(not os.path.exists(os.path.join(CSRC, so)) for so in list(FORMS.values()) + ["libfftprobe_prim.so"]):
        subprocess.check_call(["make", "-C", CSRC])
    from passiveradar_amd import _lib
    _lib.lib()                              # one HIP runtime per process (loads torch's copy first when present)
    handles = {}

    def handle(form):
        if form not in handles:
            h = ctypes.CDLL(os.path.join(CSRC, FORMS[form]))
            fn = h.fft_probe if _is_team(form) else h.fft_probe_wave
            fn.restype = ctypes.c_int
            fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
            # the library is the flag set its id says
            if _is_team(form):
                assert h.fft_probe_flags() == TEAM_FLAGS[form], (form, hex(h.fft_probe_flags()))
            else:
                assert h.fft_probe_wave_packed() == (1 if form == "wave_pk" else 0)
            handles[form] = fn
        return handles[form]

    def call(form, mode, x, y=None):
        x = np.ascontiguousarray(x, np.complex64)
        y = x if y is None else np.ascontiguousarray(y, np.complex64)
        assert x.ndim == 2 and x.shape[1] == _P(form) and y.shape == x.shape
        out = np.empty_like(x)
        rc = handle(form)(x.ctypes.data, y.ctypes.data, out.ctypes.data, x.shape[0], mode)
        if rc in (-3, -4):                  # the launch or the device failed: nothing more runs on it from this module
            pytest.exit("fft probe %s mode %d: HIP error %d" % (form, mode, rc), returncode=3)
        assert rc == 0, (form, mode, rc)
        return out
    yield call
    for cache in (_NOISE_IN, _NOISE_OUT, _REF, _W):
        cache.clear()


_NOISE_IN = {}
_NOISE_OUT = {}
_REF = {}


def _noise_in(P):
    """the shared noise inputs: u, v (time) -- also read as spectra in the frequency layout by the inverse modes"""
    if P not in _NOISE_IN:
        rng = np.random.default_rng(20240 + P)
        u = (rng.standard_normal((NOISE, P)) + 1j * rng.standard_normal((NOISE, P))).astype(np.complex64)
        v = (rng.standard_normal((NOISE, P)) + 1j * rng.standard_normal((NOISE, P))).astype(np.complex64)
        u.setflags(write=False)
        v.setflags(write=False)
        _NOISE_IN[P] = (u, v)
    return _NOISE_IN[P]


def _noise_out(run, form, mode, nz=16):
    """output of `mode` on the shared noise (zero tail for nz < 16), run as several copies in one launch so that more
    workgroups are in flight than the chip holds: every copy must give the same bits; the first is returned"""
    key = (form, mode, nz)
    if key not in _NOISE_OUT:
        P = _P(form)
        u, v = _noise_in(P)
        if nz < 16:
            u = u.copy()
            u[:, (P // 16) * nz:] = 0
        copies = TEAM_COPIES if _is_team(form) else WAVE_COPIES
        out = run(form, mode, np.tile(u, (copies, 1)), np.tile(v, (copies, 1))).reshape(copies, NOISE, P)
        for c in range(1, copies):
            assert np.array_equal(out[c].view(np.uint32), out[0].view(np.uint32)), (form, mode, "copy %d differs" % c)
        res = out[0].copy()
        res.setflags(write=False)
        _NOISE_OUT[key] = res
    return _NOISE_OUT[key]


def _errs(got, ref):
    d = got.astype(np.complex128) - ref
    return float(np.linalg.norm(d) / np.linalg.norm(ref)), float(np.abs(d).max() / np.abs(ref).max())


def _reference(P, what):
    """float64 reference and the yardstick's two errors against it, computed once per size"""
    import scipy.fft
    key = (P, what)
    if key not in _REF:
        u, v = _noise_in(P)
        u64, v64 = u.astype(np.complex128), v.astype(np.complex128)
        if what == "forward":
            ref = np.fft.fft(u64, axis=1)
            yard = scipy.fft.fft(u, axis=1)
        elif what == "roundtrip":
            ref = u64 * P
            yard = scipy.fft.ifft(scipy.fft.fft(u, axis=1), axis=1) * np.float32(P)
        elif what == "inverse":                                  # u read as a spectrum in the frequency layout
            spec = np.zeros((NOISE, P), np.complex128)
            spec[:, _bins(P)] = u64
            ref = np.fft.ifft(spec, axis=1) * P
            yard = scipy.fft.ifft(spec.astype(np.complex64), axis=1) * np.float32(P)
        else:
            ref = np.fft.ifft(3 * np.conj(np.fft.fft(u64, axis=1)) * np.fft.fft(v64, axis=1), axis=1) * P
            yard = scipy.fft.ifft(np.float32(3) * np.conj(scipy.fft.fft(u, axis=1)) * scipy.fft.fft(v, axis=1), axis=1) * np.float32(P)
        assert yard.dtype == np.complex64                        # the yardstick computes in single precision
        _REF[key] = (ref, _errs(yard, ref))
    return _REF[key]


def _hold_to_yardstick(got, P, what, label):
    ref, (y_rms, y_max) = _reference(P, what)
    rms, mx = _errs(got, ref)
    print("FIGURES_MEASURED %s %s: rms %.3g = %.2f x yardstick, max/peak %.3g = %.2f x yardstick"
          % (label, what, rms, rms / y_rms, mx, mx / y_max))
    assert rms <= YARDSTICK_FACTOR * y_rms, (label, what, rms, y_rms)
    assert mx <= YARDSTICK_FACTOR * y_max, (label, what, mx, y_max)


def _fwd_modes(form):
    return TEAM_FWD if _is_team(form) else WAVE_FWD


def _inv_modes(form):
    return TEAM_INV if _is_team(form) else WAVE_INV


def _sched_modes(form):
    return TEAM_SCHED if _is_team(form) else WAVE_SCHED


def _cases(table):
    return [pytest.param(f, m, id="%s-%s" % (f, m)) for f in TEAM_IDS + WAVE_IDS for m in table(f)]


_W = {}


def _roots(P):
    if P not in _W:
        _W[P] = np.exp(-2j * np.pi * np.arange(P) / P)
    return _W[P]


def _impulse_max_error(got, P, rows, cols, conj):
    """max | got[i, c] - W_P^(rows[i] cols[c]) | (conjugated for the inverse), expected values made in row blocks"""
    W = np.conj(_roots(P)) if conj else _roots(P)
    worst = 0.0
    for i0 in range(0, len(rows), 256):
        idx = (rows[i0:i0 + 256, None].astype(np.int64) * cols[None, :]) % P
        worst = max(worst, float(np.abs(got[i0:i0 + 256] - W[idx]).max()))
    return worst


# ---- a: every impulse through every forward form ------------------------------------------------------------------------
@pytest.mark.parametrize("form,name", _cases(_fwd_modes))
def test_every_impulse_forward(run, form, name):
    P = _P(form)
    mode, nz = _fwd_modes(form)[name]
    n = (P // 16) * nz                      # a zero-tail form takes the impulses of the samples it reads
    x = np.zeros((n, P), np.complex64)
    x[np.arange(n), np.arange(n)] = 1
    got = run(form, mode, x)
    e = _impulse_max_error(got, P, np.arange(n), _bins(P), conj=False)
    print("FIGURES_MEASURED %s %s: impulse max error %.3g" % (form, name, e))
    assert e <= IMPULSE_BAR, (form, name, e)


# ---- b: a unit spectrum line at every place of the frequency layout through every inverse form --------------------------
@pytest.mark.parametrize("form,name", _cases(_inv_modes))
def test_every_impulse_through_the_inverse(run, form, name):
    P = _P(form)
    x = np.zeros((P, P), np.complex64)
    x[np.arange(P), np.arange(P)] = 1       # input i: the line at layout element i, bin _bins(P)[i]
    got = run(form, _inv_modes(form)[name], x)
    e = _impulse_max_error(got, P, _bins(P), np.arange(P), conj=True)
    print("FIGURES_MEASURED %s %s: impulse max error %.3g" % (form, name, e))
    assert e <= IMPULSE_BAR, (form, name, e)


# ---- c: noise against the yardstick ----------------------------------------------------------------------------------
@pytest.mark.parametrize("form,name", _cases(lambda f: [m for m, (_, nz) in _fwd_modes(f).items() if nz == 16]))
def test_forward_noise_within_three_times_scipy_complex64(run, form, name):
    P = _P(form)
    got = _noise_out(run, form, _fwd_modes(form)[name][0])
    nat = np.empty_like(got)
    nat[:, _bins(P)] = got
    _hold_to_yardstick(nat, P, "forward", "%s %s" % (form, name))


@pytest.mark.parametrize("form,name", _cases(_inv_modes))
def test_inverse_noise_within_three_times_scipy_complex64(run, form, name):
    _hold_to_yardstick(_noise_out(run, form, _inv_modes(form)[name]), _P(form), "inverse", "%s %s" % (form, name))


@pytest.mark.parametrize("form", TEAM_IDS + WAVE_IDS)
def test_inverse_of_forward_noise_within_three_times_scipy_complex64(run, form):
    got = _noise_out(run, form, TEAM_ROUNDTRIP if _is_team(form) else WAVE_ROUNDTRIP)
    _hold_to_yardstick(got, _P(form), "roundtrip", form)


@pytest.mark.parametrize("form,name", _cases(_sched_modes))
def test_kernel_schedule_noise_within_three_times_scipy_complex64(run, form, name):
    """(fwd, fwd, cmac_conj_a) x 3, inverse -- twice, with the barriers the headers prescribe and no other"""
    _hold_to_yardstick(_noise_out(run, form, _sched_modes(form)[name]), _P(form), "schedule", "%s %s" % (form, name))


# ---- d: bit identity where the project claims it -----------------------------------------------------------------------
def _all_modes(form):
    """(name, mode, nz) of every mode of a form"""
    out = [(n, m, nz) for n, (m, nz) in _fwd_modes(form).items()]
    out += [(n, m, 16) for n, m in _inv_modes(form).items()]
    out += [("roundtrip", TEAM_ROUNDTRIP if _is_team(form) else WAVE_ROUNDTRIP, 16)]
    out += [(n, m, 16) for n, m in _sched_modes(form).items()]
    return out


IDENTICAL = [("wave_pk", "wave_scalar"),                                   # packed = scalar
             ("team_pk_nbuf2", "team_scalar_nbuf2"), ("team_pk_nbuf1", "team_scalar_nbuf1"),
             ("team_pk_nbuf1_tw2regs14", "team_pk_nbuf1"),                 # two T2 twiddles read from LDS = all in registers
             ("team_scalar_nbuf1", "team_scalar_nbuf2"), ("team_pk_nbuf1", "team_pk_nbuf2")]   # one buffer = two


@pytest.mark.parametrize("a,b", IDENTICAL, ids=["%s=%s" % p for p in IDENTICAL])
def test_forms_claimed_identical_give_the_same_bits(run, a, b):
    differ = []
    for name, mode, nz in _all_modes(a):
        ga, gb = _noise_out(run, a, mode, nz), _noise_out(run, b, mode, nz)
        if not np.array_equal(ga.view(np.uint32), gb.view(np.uint32)):
            differ.append((name, int((ga.view(np.uint32) != gb.view(np.uint32)).sum()), float(np.abs(ga - gb).max())))
    assert not differ, differ


# ---- e: zero tails -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,name", _cases(lambda f: [m for m, (_, nz) in _fwd_modes(f).items() if nz < 16]))
def test_zero_tail_forms_equal_the_full_form(run, form, name):
    mode, nz = _fwd_modes(form)[name]
    full = name.split("_nz")[0] if _is_team(form) else "fft1024_fwd_16"
    want = _noise_out(run, form, _fwd_modes(form)[full][0], nz)          # the same zero-tailed input through the NZ = 16 form
    got = _noise_out(run, form, mode, nz)
    assert np.abs(want).max() > 1 and np.array_equal(got, want), (form, name, float(np.abs(got - want).max()))


# ---- f: PRESCALED ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", WAVE_IDS)
def test_prescaled_inverse_equals_the_plain_inverse_bit_for_bit(run, form):
    a = _noise_out(run, form, WAVE_INV["fft1024_inv"])
    b = _noise_out(run, form, WAVE_INV["fft1024_inv_prescaled"])
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), float(np.abs(a - b).max())


# ---- g: repeatability --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,name", _cases(_sched_modes))
def test_kernel_schedule_repeats_bit_for_bit(run, form, name):
    P = _P(form)
    u, v = _noise_in(P)
    first = _noise_out(run, form, _sched_modes(form)[name])
    copies = TEAM_COPIES if _is_team(form) else WAVE_COPIES
    again = run(form, _sched_modes(form)[name], np.tile(u, (copies, 1)), np.tile(v, (copies, 1)))
    for c in range(copies):
        assert np.array_equal(again[c * NOISE:(c + 1) * NOISE].view(np.uint32), first.view(np.uint32)), (form, name, c)


# ---- the packed primitives of fft_pk.h against the scalar forms ---------------------------------------------------------
def _dft16_ref(x, sign, nz):
    x = x.copy()
    x[:, nz:] = 0
    return np.fft.fft(x, axis=1) if sign > 0 else np.fft.ifft(x, axis=1) * 16


def _running(x, c, term):
    acc = x[:, 0].copy()
    out = np.empty_like(x)
    for r in range(16):
        acc = acc + term(x[:, r], c[:, r])
        out[:, r] = acc
    return out


W_UNIFORM = 0.6 - 0.8j
# name -> (probe's number, float64 reference of the operation on registers x, per-register operand c, uniform operand w)
PRIMITIVES = {
    "dft16_fwd_16_vs_pk_dft16": (0, lambda x, c, w: _dft16_ref(x, 1, 16)),
    "dft16_fwd_12_vs_pk_dft16": (1, lambda x, c, w: _dft16_ref(x, 1, 12)),
    "dft16_fwd_8_vs_pk_dft16": (2, lambda x, c, w: _dft16_ref(x, 1, 8)),
    "dft16_inv_16_vs_pk_dft16": (3, lambda x, c, w: _dft16_ref(x, -1, 16)),
    "dft16_inv_12_vs_pk_dft16": (4, lambda x, c, w: _dft16_ref(x, -1, 12)),
    "dft16_inv_8_vs_pk_dft16": (5, lambda x, c, w: _dft16_ref(x, -1, 8)),
    "mul_tw_fwd_vs_pk_mul_tw_vgpr": (6, lambda x, c, w: x * c),
    "mul_tw_inv_vs_pk_mul_tw_vgpr": (7, lambda x, c, w: x * np.conj(c)),
    "mul_tw_fwd_vs_pk_mul_tw_sgpr": (8, lambda x, c, w: x * w),
    "mul_tw_inv_vs_pk_mul_tw_sgpr": (9, lambda x, c, w: x * np.conj(w)),
    "mul_tw_fwd_vs_pk_twiddle": (10, lambda x, c, w: np.concatenate([x[:, :1], x[:, 1:] * c[:, 1:]], axis=1)),
    "mul_tw_inv_vs_pk_twiddle": (11, lambda x, c, w: np.concatenate([x[:, :1], x[:, 1:] * np.conj(c[:, 1:])], axis=1)),
    "cmac_conj_a_vs_pk_cmac_conj_a": (12, lambda x, c, w: _running(x, c, lambda a, b: np.conj(a) * b)),
    "cmul_vs_pk_cmulc_vgpr": (13, lambda x, c, w: x * c),
    "cmul_vs_pk_cmulc_sgpr": (14, lambda x, c, w: x * w),
    "ltc_cmac_bconj_vs_pk_cmac_bconj": (15, lambda x, c, w: _running(x, c, lambda a, b: a * np.conj(b))),
    "cscale_vs_pk_scale": (16, lambda x, c, w: x * w.real),
}


@pytest.fixture(scope="module")
def prim(run):
    h = ctypes.CDLL(os.path.join(CSRC, "libfftprobe_prim.so"))
    h.fft_probe_prim.restype = ctypes.c_int
    h.fft_probe_prim.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int, ctypes.c_float, ctypes.c_float, ctypes.c_int]
    n = 4096 + 37                            # 17 workgroups, the last one ragged
    rng = np.random.default_rng(77)
    x = (rng.standard_normal((n, 16)) + 1j * rng.standard_normal((n, 16))).astype(np.complex64)
    c = (rng.standard_normal((n, 16)) + 1j * rng.standard_normal((n, 16))).astype(np.complex64)
    # signed zeros, an infinity-free spread of magnitudes and exact cancellations in the first threads
    x[0] = 0
    x[1] = -x[1] * 0
    x[2] = x[2] * np.float32(2.0 ** 40)
    x[3] = x[3] * np.float32(2.0 ** -40)
    c[4] = x[4]
    x[5, 8:] = x[5, :8]

    def call(which):
        s = np.full_like(x, np.nan)
        p = np.full_like(x, np.nan)
        rc = h.fft_probe_prim(x.ctypes.data, c.ctypes.data, s.ctypes.data, p.ctypes.data, n,
                              W_UNIFORM.real, W_UNIFORM.imag, which)
        assert rc == 0, rc
        return s, p
    return x, c, call


@pytest.mark.parametrize("name", list(PRIMITIVES))
def test_packed_primitive_rounds_exactly_as_the_scalar_form(prim, name):
    x, c, call = prim
    which, ref = PRIMITIVES[name]
    s, p = call(which)
    want = ref(x.astype(np.complex128), c.astype(np.complex128), np.complex128(np.complex64(W_UNIFORM)))
    # the scalar form is the operation it is named after: at most 17 terms of size max|x| max(1, |c|, |w|) per output, each
    # a few roundings of 2^-24 (a wrong sign or operand is an error of the size of a term) ...
    term = np.abs(x).max(axis=1, keepdims=True) * np.maximum(1.0, np.abs(c).max(axis=1, keepdims=True))
    assert np.isfinite(s.view(np.float32)).all()
    assert (np.abs(s - want) <= 17 * 4 * 2.0 ** -24 * term).all(), float((np.abs(s - want) / np.maximum(term, 1e-30)).max())
    # ... and the packed form gives its bits
    bad = s.view(np.uint32) != p.view(np.uint32)
    assert not bad.any(), (name, int(bad.sum()), float(np.abs(s - p).max()))
