"""Plain NumPy restatement of simple_target_tracker (target_detection.py:530-681) and persistence (plotting_tools.py),
rule by rule, as csrc/simple_track.hip and csrc/persistence.hip implement them.  tests/test_simple_tracker_host.py holds
it to the reference's goldens; the GPU tests hold the device to it."""
import numpy as np

# simple_target_tracker's constants (:640-647)
F1 = np.array([[1, 0, -0.003, 0], [0, 0, -0.003, -0.03], [0, 0, 1, 1], [0, 0, 0, 1]], dtype=np.float64)
F2 = np.array([[1, 1, 0, 0], [0, 1, 0, 0], [0, 0, 1, 1], [0, 0, 0, 1]], dtype=np.float64)
Q = np.diag([2.0, 0.02, 0.2, 0.05])
HM = np.array([[1, 0, 0, 0], [0, 0, 1, 0]], dtype=np.float64)
R = np.diag([5.0, 5.0])
P0 = np.diag([5.0, 0.0225, 0.04, 0.1])
X0 = np.array([30.0, 2.0, -20.0, -1.0])

# lock state transitions: state -> next state when the target is found / not found
FOUND = {0: 1, 1: 2, 2: 2, 3: 2}
LOST = {0: 0, 1: 0, 2: 3, 3: 0}
# gate half-sizes (range rows, Doppler columns) per lock state; state 0 has no gate
GATE = {1: (24, 48), 2: (16, 32), 3: (24, 48)}


def initial_state():
    """the state before frame 0.  The reference builds its record in the wrong field order, so measurement = H x0,
    measurement_idx = [35, -30] and estimate = [50, 50]"""
    return dict(lock_mode=np.array([1.0, 0, 0, 0]), measurement=HM @ X0, measurement_idx=np.array([35, -30]),
                estimate=np.array([50.0, 50.0]), x=X0.copy(), P=P0.copy(), S=np.eye(2))


def mask(W, H):
    """cells of s = fliplr(frame.T) (shape (W, H)) the reference zeroes: rows [:8] and [-8:], columns [250:260], with
    Python slice rules (W <= 16: every row; H <= 250: no column)"""
    m = np.zeros((W, H), dtype=bool)
    m[:8, :] = True
    m[-8:, :] = True
    m[:, 250:260] = True
    return m


def lock_gate(lock):
    """the gate half-sizes: lock_mode[1] == 1 first, then [2], then [3], as the reference tests them"""
    for st in (1, 2, 3):
        if lock[st] == 1:
            return GATE[st]
    return None


def window(ly, lx, half, W, H):
    """the gate's rows and columns after Python slice normalisation (a negative start wraps to n + start, then clips)"""
    dy, dx = half
    r = slice(int(ly) - dy, int(ly) + dy).indices(W)[:2]
    c = slice(int(lx) - dx, int(lx) + dx).indices(H)[:2]
    return r, c


def argmax_index(frame, lock, ly, lx):
    """np.argmax(s * gate) of one (H, W) frame, by the frame's class:
    * a NaN in the frame or all zeros: every cell is NaN after the division, the first unmasked cell wins;
    * an Inf in the frame: the unmasked +-Inf cells are Inf/Inf = NaN under any gate, the first wins; else all +-0;
    * positive finite mean: the first largest raw value inside the gate if it is > 0, else s[0, 0] (always a masked
      zero).  Division by the positive mean keeps the order of float32 values, so raw values are compared."""
    H, W = frame.shape
    v = np.asarray(frame, dtype=np.float64)
    s = np.fliplr(v.T)
    m = mask(W, H)
    total = np.sum(np.abs(v))
    if np.isnan(total) or total == 0:
        free = np.flatnonzero(~m)
        return divmod(int(free[0]), H) if free.size else (0, 0)
    if np.isinf(total / v.size):
        nan_cells = np.flatnonzero(np.isinf(s) & ~m)
        return divmod(int(nan_cells[0]), H) if nan_cells.size else (0, 0)
    inside = ~m
    half = lock_gate(lock)
    if half is not None:
        (r0, r1), (c0, c1) = window(ly, lx, half, W, H)
        g = np.zeros((W, H), dtype=bool)
        g[r0:r1, c0:c1] = True
        inside &= g
    vals = np.where(inside, s, -np.inf)
    j = int(np.argmax(vals))
    return divmod(j, H) if vals.flat[j] > 0 else (0, 0)


def kalman(x, P, z, last_z):
    """adaptive_kalman_update (:63-114): R scaled by the squared distance to the previous measurement"""
    d = z - last_z
    x = F1 @ x
    P = F2 @ P @ F2.T + Q
    S = HM @ P @ HM.T + R * (d[0] ** 2 + d[1] ** 2)
    K = P @ HM.T @ np.linalg.inv(S)
    x = x + K @ (z - HM @ x)
    P = (np.eye(4) - K @ HM) @ P
    return x, P, S


def badness(z, estimate):
    d = z - estimate
    return float(np.sqrt(d[0] ** 2 + (0.5 * d[1]) ** 2))


def step(state, frame, range_extent, doppler_extent):
    H, W = frame.shape
    lock = state["lock_mode"]
    i0, i1 = argmax_index(frame, lock, state["measurement_idx"][0], state["measurement_idx"][1])
    # measurement: this float64 operation order
    z = np.array([range_extent * (1 - i0 / W), doppler_extent * (2 * i1 / H - 1)])
    b = badness(z, state["estimate"])
    table = FOUND if b < 12 else LOST
    new_lock = np.zeros(4)
    for st in range(4):
        new_lock[table[st]] += lock[st]
    x, P, S = kalman(state["x"], state["P"], z, state["measurement"])
    return dict(lock_mode=new_lock, measurement=z, measurement_idx=np.array([i0, i1]), estimate=HM @ x, x=x, P=P,
                S=S), b


def simple_target_tracker(data, range_extent, doppler_extent, state=None):
    """data (H, W, N); returns a dict of (N, ...) arrays and each frame's badness"""
    st = initial_state() if state is None else {k: np.array(v) for k, v in state.items()}
    out = {k: [] for k in ("lock_mode", "measurement", "measurement_idx", "estimate", "x", "P", "S")}
    bad = []
    for i in range(data.shape[2]):
        st, b = step(st, data[:, :, i], range_extent, doppler_extent)
        bad.append(b)
        for k in out:
            out[k].append(st[k])
    res = {k: np.array(v) for k, v in out.items()}
    res["P"] = res["P"].reshape(-1, 16)
    res["S"] = res["S"].reshape(-1, 4)
    res["badness"] = np.array(bad)
    return res


def persistence(X, k, hold, decay, weak=True):
    """sum_{i < min(k+1, hold)} X[:, :, k-i] * decay**i from +0.0, term by term.  decay**i is Python's float power
    (libm pow); a float32 X with a Python-scalar decay (``weak``) forms float32 products (NumPy >= 2, NEP 50), which
    are then added in float64"""
    out = np.zeros((X.shape[0], X.shape[1]))
    n = min(k + 1, hold)
    if n > 0 and k >= X.shape[2]:
        raise IndexError(f"index {k} is out of bounds for axis 2 with size {X.shape[2]}")
    for i in range(max(n, 0)):
        p = float(decay) ** i
        x = X[:, :, k - i]
        if x.dtype == np.float32 and weak:
            term = x * np.float32(p)
        else:
            term = x.astype(np.float64) * p
        out = out + term
    return out
