"""Without a GPU: (1) every set of FT_* defines that passiveradar_amd/csrc/Makefile ships a register / LDS transform with
has a probe library in tests/csrc/Makefile (tests/test_gpu_fft_forms.py runs those probes); (2) the twiddle tables the
library builds on the host (fftw_make_tables, ft_make_tables -- reached through tests/csrc/libffttables.so, which links
against libprcore) hold cos / sin of the documented angles, rounded once."""
import ctypes
import os
import re
import subprocess

import numpy as np

from conftest import REPO

CSRC = os.path.join(REPO, "passiveradar_amd", "csrc")
PROBES = os.path.join(REPO, "tests", "csrc")


# ---- flag sets --------------------------------------------------------------------------------------------------------
def _make_vars(path, prefix):
    """{name: [tokens]} of the `<prefix><name> = ...` lines of a Makefile"""
    out = {}
    for ln in open(path).read().splitlines():
        m = re.match(r"^%s(\w+)\s*=\s*(.*)$" % re.escape(prefix), ln)
        if m:
            out[m.group(1)] = m.group(2).split()
    return out


def _ft_defines(tokens):
    """the FT_* defines of a flag list as a dict (a bare -DNAME is '1')"""
    d = {}
    for tok in tokens:
        m = re.match(r"^-D(FT_\w+)(?:=(\w+))?$", tok)
        if m:
            d[m.group(1)] = m.group(2) or "1"
    return d


def _team_key(d, nbuf_default):
    """a team flag set with the header's defaults filled in: (PK, NBUF, TW2_REGS, FACTORED)"""
    assert set(d) <= {"FT_PK", "FT_NBUF", "FT_TW2_REGS", "FT_TW2_FACTORED"}, "a define this guard does not know: %r" % d
    return ("FT_PK" in d, int(d.get("FT_NBUF", nbuf_default)), int(d.get("FT_TW2_REGS", 16)), "FT_TW2_FACTORED" in d)


def _transform_of(unit_src, seen=None):
    """'team', 'wave' or None: which of the two probed transforms a translation unit compiles (fft_team8.h has its own
    probe, doppler_col.h is emulated on the CPU: tests/test_gpu_fft_team.py, tests/test_host_logic.py)"""
    seen = seen if seen is not None else set()
    text = open(unit_src).read()
    incs = [i for i in re.findall(r'^#include "([\w.]+)"', text, flags=re.M) if i not in seen]
    seen.update(incs)
    kinds = set()
    for inc in incs:
        if inc == "fft_team.h":
            kinds.add("team")
        elif inc in ("fft_wave.h", "fft_wave_pk.h", "fft_pk.h"):
            kinds.add("wave")
        elif inc in ("fft_team8.h", "doppler_col.h"):
            continue
        elif os.path.exists(os.path.join(CSRC, inc)):
            k = _transform_of(os.path.join(CSRC, inc), seen)
            if k:
                kinds.add(k)
    return "team" if "team" in kinds else ("wave" if "wave" in kinds else None)


def _shipped_sets():
    """[(unit, kind, defines as the Makefile states them, the unit's own FT_NBUF default or None)] for every unit of
    libprcore that compiles one of the two transforms"""
    flags = _make_vars(os.path.join(CSRC, "Makefile"), "F_")
    srcs = _make_vars(os.path.join(CSRC, "Makefile"), "")["SRCS"]
    out = []
    for src in srcs:
        unit = src[:-len(".hip")]
        path = os.path.join(CSRC, src)
        text = open(path).read()
        if not re.search(r"\b(ft4096_(fwd|inv)|fft1024_(fwd|inv))\s*[<(]", text):
            continue
        kind = _transform_of(path)
        assert kind, unit
        m = re.search(r"#ifndef FT_NBUF\s*\n\s*#define FT_NBUF (\d+)", text)
        out.append((unit, kind, _ft_defines(flags.get(unit, [])), int(m.group(1)) if m else None))
    return out


def test_every_shipped_flag_set_of_the_transforms_has_a_probe():
    probes = _make_vars(os.path.join(PROBES, "Makefile"), "P_")
    lists = _make_vars(os.path.join(PROBES, "Makefile"), "")
    team = {_team_key(_ft_defines(probes[so[:-3]]), 2) for so in lists["TEAM_PROBES"]}
    wave = {"FT_PK" in _ft_defines(probes[so[:-3]]) for so in lists["WAVE_PROBES"]}
    # build() makes the default target: every probe is part of it
    all_line = re.search(r"^all:(.*)$", open(os.path.join(PROBES, "Makefile")).read(), flags=re.M).group(1).split()
    assert "$(TEAM_PROBES)" in all_line and "$(WAVE_PROBES)" in all_line and "libfftprobe_prim.so" in all_line
    shipped = _shipped_sets()
    units = {u for u, _, _, _ in shipped}
    # the guard sees the units it is about (a rename must not empty it)
    assert {"caf_fft", "ls_fft", "caf_fft_team", "caf_fft_team_multi", "ls_fft_team", "ls_fft_team_cached",
            "ls_fft_team_corr_cached"} <= units, units
    missing = []
    for unit, kind, d, own_nbuf in shipped:
        if kind == "wave":
            assert set(d) <= {"FT_PK"}, (unit, d)
            if ("FT_PK" in d) not in wave:
                missing.append((unit, d))
            continue
        # as the Makefile states it (no FT_NBUF: the header's default, two buffers) ...
        if _team_key(d, 2) not in team:
            missing.append((unit, d))
        # ... and as the unit compiles it (a unit may set its own default before it includes fft_team.h)
        if own_nbuf is not None and _team_key(d, own_nbuf) not in team:
            missing.append((unit, dict(d, FT_NBUF_default_of_the_unit=own_nbuf)))
    assert not missing, "shipped flag sets without a probe in tests/csrc/Makefile: %r" % missing
    # compiler flags that decide roundings are those of the shipped build
    ship = _make_vars(os.path.join(CSRC, "Makefile"), "")["CXXFLAGS"]
    mine = lists["FLAGS"]
    for f in ("-O3", "-fno-fast-math", "-ffp-contract=on", "-fno-slp-vectorize"):
        assert f in ship and f in mine, f


def test_the_guard_reads_defines_and_defaults_as_meant():
    assert _ft_defines("-DFT_NBUF=1 -DFT_PK -DFT_TW2_REGS=14 -mllvm -O3".split()) == {"FT_NBUF": "1", "FT_PK": "1", "FT_TW2_REGS": "14"}
    assert _team_key({}, 2) == (False, 2, 16, False)
    assert _team_key({"FT_PK": "1"}, 1) == (True, 1, 16, False)
    assert _team_key({"FT_PK": "1", "FT_NBUF": "2", "FT_TW2_FACTORED": "1"}, 1) == (True, 2, 16, True)
    kinds = {u: k for u, k, _, _ in _shipped_sets()}
    assert kinds["ls_fft"] == "wave" and kinds["caf_fft"] == "wave"
    assert kinds["ls_fft_team_cached"] == "team" and kinds["caf_fft_team"] == "team"
    assert "caf_fft_team8" not in kinds and "caf_doppler" not in kinds


# ---- tables -----------------------------------------------------------------------------------------------------------
def _library_tables():
    lib = os.path.join(PROBES, "libffttables.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-C", PROBES, "libffttables.so"])
    from passiveradar_amd import _lib
    _lib.lib()
    h = ctypes.CDLL(lib)
    h.fft_probe_tables.restype = ctypes.c_int
    h.fft_probe_tables.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    sizes = h.fft_probe_tables(None, None)
    nw, nt = sizes & 0xFFFF, sizes >> 16
    wave = np.full(nw + 8, np.nan + 0j, np.complex64)            # eight guard elements behind each table
    team = np.full(nt + 8, np.nan + 0j, np.complex64)
    assert h.fft_probe_tables(wave.ctypes.data, team.ctypes.data) == sizes
    assert np.isnan(wave[nw:].real).all() and np.isnan(team[nt:].real).all()
    return wave[:nw], team[:nt]


def _assert_unit_roots(got, num, den, what):
    ang = -2.0 * np.pi * num.astype(np.float64) / den
    for part, want in ((got.real, np.cos(ang)), (got.imag, np.sin(ang))):
        err = np.abs(part.astype(np.float64) - want)
        assert err.max() <= 2.0 ** -24, (what, float(err.max()))
        # "double-precision trig, rounded once" (fft_wave.h, fft_team.h): every entry is the float32 NEAREST to the float64
        # value -- within half a unit in the last place of the entry itself, which a float32 sincosf does not deliver and
        # which the absolute bound above cannot see for the small entries.  (The 1e-6 of slack is 2^20 roundings of a double.)
        half_ulp = 0.5 * np.spacing(np.maximum(np.abs(part), np.float32(2.0 ** -126))).astype(np.float64)
        assert (err <= half_ulp * (1 + 1e-6)).all(), (what, int((err > half_ulp * (1 + 1e-6)).sum()))


def test_twiddle_tables_of_the_library_hold_the_documented_roots_of_unity():
    wave, team = _library_tables()
    assert wave.size == 16 * 64 + 16 * 4 + 16 * 4 and team.size == 256 + 4096
    assert np.isfinite(wave.view(np.float32)).all() and np.isfinite(team.view(np.float32)).all()
    # fft_wave.h: TW1 [k1][n2] = W_1024^(n2 k1); TW2 [m'][j] = W_64^(j m'); TW2S = TW2 times the quad sign sA_j sB_j
    k1, n2 = np.meshgrid(np.arange(16), np.arange(64), indexing="ij")
    _assert_unit_roots(wave[:1024].reshape(16, 64), k1 * n2, 1024.0, "wave TW1")
    m, j = np.meshgrid(np.arange(16), np.arange(4), indexing="ij")
    tw2, tw2s = wave[1024:1088].reshape(16, 4), wave[1088:].reshape(16, 4)
    _assert_unit_roots(tw2, m * j, 64.0, "wave TW2")
    sA = np.where(np.arange(4) < 2, 1.0, -1.0)                  # fft_lane_setup(): lanes 0, 1 of a quad / lanes 2, 3
    sB = np.where(np.arange(4) & 1, -1.0, 1.0)                  # even / odd lanes of a quad
    want = (tw2 * (sA * sB).astype(np.float32)[None, :]).astype(np.complex64)
    assert np.array_equal(tw2s.view(np.uint32) & 0x7FFFFFFF, want.view(np.uint32) & 0x7FFFFFFF)      # same magnitudes, bit for bit
    assert np.array_equal(tw2s, want)                                                                # and the signs (-0 == +0)
    # fft_team.h: TW1 [k1][n2] = W_256^(n2 k1), then W_4096^m
    k1, n2 = np.meshgrid(np.arange(16), np.arange(16), indexing="ij")
    _assert_unit_roots(team[:256].reshape(16, 16), k1 * n2, 256.0, "team TW1")
    _assert_unit_roots(team[256:], np.arange(4096), 4096.0, "team W_4096")
