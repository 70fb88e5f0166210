"""Seeded random-shape sweep of the entry points added after kind 25 of tests/fuzz_parity.py, on the GPU, against their oracles
(tests/sweep_cases.py has the kinds, the case generators and the bars; tests/test_sweep_host.py holds the lists to every switch
point).  Header section of include/prcore.h -> kind:

    LS_Filter_SVD -> ls_svd | ECA_Filter -> eca | GAL_JPE -> gal | order-statistic CFAR -> cfar_os | target tracking -> track |
    plot extraction -> plots | track-before-detect -> tbd | single-target tracker -> strack | persistence -> persistence |
    display frames -> display | Welch spectra -> welch | FIR decimator and the rest of signal_utils.py -> preproc |
    exact cross-ambiguity patches -> patch | joint least-squares removal of strong echoes -> echo

test_sweep runs a kind's 24 cases in a seeded shuffled order (sizes rise and fall through the per-thread staging buffers) and
holds each to its oracle at the bar of the kind's own GPU test.  test_sweep_order_and_position runs them again in the reverse
order, then every frame / block / stream / channel / patch alone and the stack reversed, caller-owned workspaces holding 0x00 in
one pass and 0xFF in the other, plots also on the other storage path: every byte equals the first pass.  test_sweep_four_threads
runs six cases per kind from four caller threads at once, each thread on its own workspaces and in its own order: every byte
equals the single-threaded pass."""
import threading
import time
import zlib

import numpy as np
import pytest

import sweep_cases as SC

pytestmark = pytest.mark.gpu

KIND_NAMES = list(SC.KINDS)
_FIRST = {}


def visiting_order(kind, salt=0):
    return [int(i) for i in np.random.default_rng([SC.SEED, salt, zlib.crc32(kind.encode())]).permutation(SC.NCASES)]


def first_pass(kind):
    """(cases, results in case order, failures): the kind's cases run once, in the shuffled order, shared by the tests"""
    if kind not in _FIRST:
        cases = SC.cases(kind)
        results, failures = [None] * len(cases), []
        for i in visiting_order(kind):
            results[i] = SC.run(cases[i])
            try:
                SC.check(cases[i], results[i])
            except AssertionError as e:
                failures.append(str(e))
        _FIRST[kind] = (cases, results, failures)
    return _FIRST[kind]


@pytest.mark.parametrize("kind", KIND_NAMES)
def test_sweep(gpu_ready, kind):
    cases, results, failures = first_pass(kind)
    assert len(cases) == SC.NCASES and all(r is not None for r in results)
    assert not failures, f"{len(failures)} of {len(cases)} {kind} cases miss their oracle:\n" + "\n".join(failures)


def differing(a, b):
    """the names of the parts of two per-frame tuples whose bytes differ"""
    return [j for j, (u, v) in enumerate(zip(a, b)) if SC.to_bytes(u) != SC.to_bytes(v)] if len(a) == len(b) else ["length"]


@pytest.mark.parametrize("kind", KIND_NAMES)
def test_sweep_order_and_position(gpu_ready, kind):
    k = SC.KINDS[kind]
    cases, results, _ = first_pass(kind)
    failures = []
    for i in reversed(visiting_order(kind)):
        c, base = cases[i], results[i]
        again = SC.run(c, fill=0x00)
        if SC.to_bytes(again) != SC.to_bytes(base):
            bad = [(f, differing(a, b)) for f, (a, b) in enumerate(zip(again["frames"], base["frames"])) if differing(a, b)]
            failures.append(f"{c!r}: run again in the reverse order, the bytes differ (frame, parts): {bad or 'whole'}")
        for order in k.orders(c):
            got = SC.run(c, order=order, fill=0xFF)["frames"]
            for pos, f in enumerate(order):
                if differing(got[pos], base["frames"][f]):
                    failures.append(f"{c!r}: frame {f} at position {pos} of {order} differs from the first pass in parts "
                                    f"{differing(got[pos], base['frames'][f])}")
        for label, frames in k.extra_passes(c, base):
            for f, (a, b) in enumerate(zip(frames, base["frames"])):
                if differing(a, b):
                    failures.append(f"{c!r}: {label}: frame {f} differs in parts {differing(a, b)}")
    assert not failures, (f"{len(failures)} {kind} results depend on call order, position or workspace contents:\n"
                          + "\n".join(failures[:12]))


def test_sweep_four_threads(gpu_ready):
    SC.preload()                                              # everything imported here, on the main thread (tests/fuzz_parity.py)
    work = [(kind, i) for kind in KIND_NAMES for i in range(SC.THREAD_CASES)]
    cases = {kind: SC.cases(kind) for kind in KIND_NAMES}
    t0 = time.time()
    single = {(kind, i): SC.to_bytes(SC.run(cases[kind][i], plain=True)) for kind, i in work}
    t_single = time.time() - t0
    current, wrong, errors = {}, [], []

    def caller(t):
        order = np.random.default_rng([SC.SEED, 4, t]).permutation(len(work))
        fill = None if t % 2 == 0 else 0x20 + t               # the NumPy front ends on their staging buffers / filled workspaces
        try:
            for j in order:
                kind, i = work[int(j)]
                current[t] = cases[kind][i]
                if SC.to_bytes(SC.run(cases[kind][i], fill=fill, plain=True)) != single[(kind, i)]:
                    wrong.append((t, cases[kind][i]))
            current[t] = None
        except Exception as e:                                # a crash in one thread is a failure, not a silent exit
            import traceback
            errors.append((t, current.get(t), f"{e!r}\n{traceback.format_exc()[-800:]}"))
    threads = [threading.Thread(target=caller, args=(t,), daemon=True) for t in range(4)]
    t0 = time.time()
    [t.start() for t in threads]
    deadline = t0 + 30.0 + 10.0 * t_single                    # four threads share one device and one interpreter: 4 x at most
    for t in threads:
        t.join(max(0.0, deadline - time.time()))
    stuck = [(n, current.get(n)) for n, t in enumerate(threads) if t.is_alive()]
    print(f"single-threaded pass of {len(work)} cases {t_single:.1f} s; four threads {time.time() - t0:.1f} s")
    assert not stuck, f"threads that did not return within {deadline - t0:.0f} s, and the case each is in: {stuck}"
    assert not errors, f"exceptions in caller threads: {errors}"
    assert not wrong, f"{len(wrong)} results differ from the single-threaded pass (thread, case): {wrong[:8]}"
