"""Every argument check a NumPy / torch front door documents raises its exception before a device is touched: neither
_lib.require_gpu nor a _lib.DeviceBuffer is reached.  One bad call per check; no GPU needed."""
import numpy as np
import pytest

EXT = [250.0, 300.0]


class FakeDeviceTensor:
    """what _lib.is_device_tensor takes for a device tensor"""
    is_cuda = True
    device = "cuda:0"
    dtype = "torch.float32"

    def __init__(self, shape):
        self.shape = tuple(shape)

    def data_ptr(self):
        return 0

    def dim(self):
        return len(self.shape)

    def is_complex(self):
        return False


def _td():
    from passiveradar_amd import target_detection
    return target_detection


def _pt():
    from passiveradar_amd import plotting_tools
    return plotting_tools


def _cr():
    from passiveradar_amd import clutter_removal
    return clutter_removal


F2 = np.ones((24, 40), np.float32)                 # a frame [H, W]
S3 = np.ones((3, 24, 40), np.float32)              # a stack [N, H, W]
X3 = np.ones((24, 40, 3), np.complex64)            # maps (H, W, N) as the scripts load them
B3 = np.zeros((3, 24, 40), np.uint8)
P3 = np.zeros((2, 3, 3), np.complex64)             # two patches
CH = np.ones(64, np.complex64)
D1, D3, D4 = FakeDeviceTensor((40,)), FakeDeviceTensor((3, 24, 40)), FakeDeviceTensor((2, 3, 24, 40))     # stand-in tensors

# (module, function, args, kwargs, exception, message)
CASES = [
    (_td, "CFAR_2D_abs", (np.ones(8, np.complex64), 8, 2), {}, ValueError, "2-D map or a stack"),
    (_td, "CFAR_2D_OS", (np.ones(8, np.float32), 18, 4), {}, ValueError, "2-D map or a stack"),
    (_td, "CFAR_2D_OS", (F2, 18, 4), dict(rank=300), ValueError, "rank"),
    (_td, "CFAR_2D_OS", (F2, 18, 4), dict(rank=0), ValueError, "rank counts from 1"),
    (_td, "CFAR_2D_OS", (F2, 18, 4), dict(scale="decibel"), ValueError, "scale is one of"),
    (_td, "CFAR_2D_OS", (F2, 1, 0), {}, ValueError, "no training cell"),
    (_td, "get_measurements", (S3, 99.8, EXT), {}, ValueError, "one 2-D frame"),
    (_td, "multitarget_tracker", (F2, EXT, 4), {}, ValueError, r"\(H, W, Nframes\)"),
    (_td, "track_maps", (X3, EXT, 4), dict(measure="clusters", plot_thresh=2.0), ValueError, "measure is"),
    (_td, "track_maps", (X3, EXT, 4), dict(measure="plots"), ValueError, "needs plot_thresh"),
    (_td, "track_maps", (X3, EXT, 4), dict(cfar="median"), ValueError, "cfar is 'mean' or 'os'"),
    (_td, "track_maps", (X3, EXT, 4), dict(cfar="median", measure="plots", plot_thresh=2.0), ValueError, "cfar is 'mean' or 'os'"),
    (_td, "track_maps", (X3[:, :, 0], EXT, 4), dict(measure="plots", plot_thresh=2.0), ValueError, r"\(H, W, Nframes\)"),
    (_td, "track_maps", (X3, EXT, 4), dict(measure="plots", plot_thresh=2.0, plot_connectivity=6), ValueError, "connectivity = 6, not 4 or 8"),
    (_td, "track_maps", (X3, EXT, 4), dict(measure="plots", plot_thresh=2.0, plot_max_cells=0), ValueError, "max_cells = 0"),
    (_td, "track_maps", (X3, EXT, 4), dict(measure="plots", plot_thresh=2.0, plot_capacity=0), ValueError, "capacity = 0"),
    (_td, "extract_plots", (np.ones(40, np.float32), 0.5, EXT), {}, ValueError, "a frame .H, W. or a stack"),
    (_td, "extract_plots", (F2, 0.5, EXT), dict(weight=np.ones((24, 41), np.float32)), ValueError, "weight has shape"),
    (_td, "extract_plots", (F2, 0.5, EXT), dict(weight=FakeDeviceTensor((24, 40))), ValueError,
     "stat and weight are both NumPy arrays or both device tensors"),
    (_td, "extract_plots", (F2, 0.5, EXT), dict(connectivity=5), ValueError, "connectivity = 5, not 4 or 8"),
    (_td, "extract_plots", (F2, 0.5, EXT), dict(range_guard=-1), ValueError, "range_guard = -1, doppler_guard = 4: not >= 0"),
    (_td, "extract_plots", (F2, 0.5, EXT), dict(doppler_guard=-1), ValueError, "range_guard = 8, doppler_guard = -1: not >= 0"),
    (_td, "extract_plots", (F2, 0.5, EXT), dict(max_cells=0), ValueError, "max_cells = 0"),
    (_td, "extract_plots", (F2, 0.5, EXT), dict(capacity=0), ValueError, "capacity = 0"),
    (_td, "extract_plots", (F2, float("nan"), EXT), {}, ValueError, "thresh is NaN"),
    (_td, "track_before_detect", (np.ones(40, np.float32),), {}, ValueError, "a frame .H, W. or a stack"),
    (_td, "track_before_detect", (S3,), dict(alpha=0.0), ValueError, r"alpha = 0, not in \(0, 1\]"),
    (_td, "track_before_detect", (S3,), dict(doppler_reach=-1), ValueError, "doppler_reach = -1, range_reach = 1: not >= 0"),
    (_td, "track_before_detect", (S3,), dict(clip=float("nan")), ValueError, "clip is NaN"),
    (_td, "track_before_detect", (S3,), dict(row_shifts=np.zeros(23, np.int32)), ValueError, "row_shifts must be 24 integers"),
    (_td, "track_before_detect", (S3,), dict(row_shifts=np.zeros(24, np.float32)), ValueError, "row_shifts must be 24 integers"),
    (_td, "track_before_detect", (S3,), dict(prev=np.zeros((24, 41), np.float32)), ValueError, "prev has shape"),
    (_td, "track_before_detect", (S3,), dict(prev=FakeDeviceTensor((24, 40))), ValueError,
     "stat and prev are both NumPy arrays or both device tensors"),
    (_td, "tbd_paths", (B3[0], [[0, 0]], 4), {}, ValueError, "back is a stack"),
    (_td, "tbd_paths", (B3, [[0, 0]], 0), {}, ValueError, "depth = 0"),
    (_td, "tbd_paths", (B3, [0, 0, 0], 4), {}, ValueError, r"ends is \[nends, 2\]"),
    (_td, "tbd_paths", (B3, [[0, 0]], 4), dict(doppler_reach=-1), ValueError, "doppler_reach = -1, range_reach = 1: not >= 0"),
    (_td, "tbd_paths", (B3, [[0, 0]], 4), dict(row_shifts=np.zeros(5, np.int32)), ValueError, "row_shifts must be 24 integers"),
    (_td, "tbd_maps", (X3, EXT, 0.5, 3.0), dict(thresh=5.0, cfar="median"), ValueError, "cfar is 'mean' or 'os'"),
    (_td, "tbd_maps", (X3[:, :, 0], EXT, 0.5, 3.0), dict(thresh=5.0), ValueError, r"\(H, W, Nframes\)"),
    (_td, "tbd_maps", (X3, EXT, 0.5, 3.0), dict(thresh=5.0, alpha=2.0), ValueError, r"alpha = 2, not in \(0, 1\]"),
    (_td, "tbd_maps", (X3, EXT, 0.5, 3.0), dict(thresh=5.0, return_back=False), TypeError, "unexpected keyword"),
    (_td, "tbd_maps", (X3, EXT, 0.5, 3.0), dict(thresh=5.0, plot_connectivity=6), ValueError, "connectivity = 6, not 4 or 8"),
    (_td, "simple_target_tracker", (F2, 10.0, 10.0), {}, ValueError, r"\(H, W, Nframes\)"),
    (_td, "simple_target_tracker", (np.ones((24, 40, 3), np.float32), 10.0, 10.0), dict(state=np.zeros(2)), ValueError,
     "state= takes one row"),
    (_td, "simple_track_maps", (X3, 10.0, 10.0), dict(cfar="median"), ValueError, "cfar is 'mean' or 'os'"),
    (_td, "refine_peaks", (P3[0], [0], [0.0], 1.0), {}, ValueError, "takes patches"),
    (_td, "refine_peaks", (P3, [0], [0.0], 1.0), {}, ValueError, "2 patches but 1 origins"),
    (_td, "refine_peaks", (P3, [0.5, 1], [0.0, 0.0], 1.0), {}, ValueError, "whole samples"),
    (_td, "refine_peaks", (P3, [0, 1], [0.0, float("inf")], 1.0), {}, ValueError, "must be finite"),
    (_pt, "persistence", (np.ones((4, 3)), 0, 2, 0.9), {}, ValueError, r"\(H, W, L\) stack"),
    (_pt, "persistence", (np.ones((4, 3, 2)), 2, 2, 0.9), {}, IndexError, "index 2 is out of bounds for axis 2 with size 2"),
    (_pt, "persistence_stack", (np.ones((4, 3)), 2, 0.9), {}, ValueError, r"\(H, W, L\) stack"),
    (_pt, "persistence_stack", (np.ones((4, 3, 2)), 2, 0.9), dict(out_dtype=np.int32), ValueError, "out_dtype is float64 or float32"),
    (_pt, "display_limits", (np.ones((4, 3)),), {}, ValueError, r"\(H, W, L\) stack"),
    (_pt, "display_limits", (np.ones((4, 3, 2)),), dict(p_lo=101), ValueError, "Percentiles must be in the range"),
    (_pt, "display_limits", (np.ones((0, 3, 2)),), {}, ValueError, "need H, W >= 1"),
    (_pt, "render_frames", (np.ones((4, 3)),), {}, ValueError, r"\(H, W, L\) stack"),
    (_pt, "render_frames", (np.ones((4, 3, 2)),), dict(p_hi=-1), ValueError, "Percentiles must be in the range"),
    (_pt, "render_frames", (np.ones((4, 3, 2)),), dict(lut=np.zeros((256, 3), np.uint8)), ValueError, "lut is a uint8"),
    (_pt, "render_frames", (np.ones((4, 3, 2)),), dict(orient="flipped"), ValueError, "orient is"),
    (_pt, "render_frames", (np.ones((4, 3, 2)),), dict(limits=np.zeros((3, 2))), ValueError, r"limits is \(L, 2\) = \(2, 2\)"),
    (_pt, "render_frames", (np.ones((4, 3, 2)),), dict(limits=np.zeros((2, 3))), ValueError, r"limits is \(L, 2\) = \(2, 2\)"),
    (_pt, "render_maps", (np.ones((4, 3)),), {}, ValueError, r"\(H, W, L\) maps"),
    (_pt, "render_maps", (np.ones((4, 3, 2)),), dict(cfar="median"), ValueError, "cfar is 'mean' or 'os'"),
    (_pt, "render_maps", (np.ones((4, 3, 2)),), dict(slab=0), ValueError, "slab is a number of frames"),
    # a device tensor first: the shape checks of the torch side, before a cast or an allocation
    (_td, "CFAR_2D_abs", (D1, 8, 2), {}, ValueError, "2-D map or a stack"),
    (_td, "CFAR_2D_OS", (D1, 18, 4), {}, ValueError, "2-D map or a stack"),
    (_td, "CFAR_2D_OS", (D3, 18, 4), dict(rank=0), ValueError, "rank counts from 1"),
    (_td, "multitarget_tracker", (D4, EXT, 4), {}, ValueError, r"multitarget_tracker takes a device stack \[N, H, W\]"),
    (_td, "track_maps", (D4, EXT, 4), {}, ValueError, r"track_maps takes a device stack \[N, H, W\]"),
    (_td, "track_maps", (D3, EXT, 4), dict(cfar="median"), ValueError, "cfar is 'mean' or 'os'"),
    (_td, "track_maps", (D3, EXT, 4), dict(measure="plots", plot_thresh=2.0, plot_capacity=0), ValueError, "capacity = 0"),
    (_td, "extract_plots", (D1, 0.5, EXT), {}, ValueError, "a frame .H, W. or a stack"),
    (_td, "extract_plots", (D3, 0.5, EXT), dict(weight=np.ones((3, 24, 40), np.float32)), ValueError,
     "stat and weight are both NumPy arrays or both device tensors"),
    (_td, "extract_plots", (D3, 0.5, EXT), dict(weight=FakeDeviceTensor((3, 24, 41))), ValueError, "weight has shape"),
    (_td, "track_before_detect", (D1,), {}, ValueError, "a frame .H, W. or a stack"),
    (_td, "track_before_detect", (D3,), dict(prev=np.zeros((24, 40), np.float32)), ValueError,
     "stat and prev are both NumPy arrays or both device tensors"),
    (_td, "track_before_detect", (D3,), dict(prev=FakeDeviceTensor((24, 41))), ValueError, "prev has shape"),
    (_td, "tbd_paths", (FakeDeviceTensor((24, 40)), [[0, 0]], 4), {}, ValueError, "back is a stack"),
    (_td, "tbd_paths", (D3, [0, 0, 0], 4), {}, ValueError, r"ends is \[nends, 2\]"),
    (_td, "tbd_maps", (D4, EXT, 0.5, 3.0), dict(thresh=5.0), ValueError, r"tbd_maps takes a device stack \[N, H, W\]"),
    (_td, "simple_target_tracker", (FakeDeviceTensor((24, 40)), 10.0, 10.0), {}, ValueError,
     r"simple_target_tracker takes a device stack \[N, H, W\]"),
    (_td, "simple_track_maps", (D4, 10.0, 10.0), {}, ValueError, r"simple_track_maps takes a device stack \[N, H, W\]"),
    (_td, "refine_peaks", (FakeDeviceTensor((3, 3)), [0], [0.0], 1.0), {}, ValueError, "takes patches"),
    (_pt, "persistence", (FakeDeviceTensor((4, 3)), 0, 2, 0.9), {}, ValueError, r"persistence takes a device stack \[L, H, W\]"),
    (_pt, "persistence", (D3, 3, 2, 0.9), {}, IndexError, "index 3 is out of bounds for axis 2 with size 3"),
    (_pt, "persistence_stack", (FakeDeviceTensor((4, 3)), 2, 0.9), {}, ValueError,
     r"persistence_stack takes a device stack \[L, H, W\]"),
    (_pt, "display_limits", (FakeDeviceTensor((4, 3)),), {}, ValueError, r"display_limits takes a device stack \[L, H, W\]"),
    (_pt, "render_frames", (FakeDeviceTensor((4, 3)),), {}, ValueError, r"render_frames takes a device stack \[L, H, W\]"),
    (_pt, "render_frames", (D3,), dict(limits=np.zeros((2, 2))), ValueError, r"limits is \(L, 2\) = \(3, 2\)"),
    (_pt, "render_maps", (FakeDeviceTensor((4, 3)),), {}, ValueError, r"render_maps takes a device stack \[L, H, W\]"),
    (_pt, "render_maps", (D3,), dict(limits=np.zeros((2, 2))), ValueError, r"limits is \(L, 2\) = \(3, 2\)"),
    (_cr, "cancel_echoes", (CH, CH[:63], 1e5, [3], [1.0]), {}, ValueError, "same length"),
    (_cr, "cancel_echoes", (np.ones((2, 2, 8), np.complex64),) * 2 + (1e5, [3], [1.0]), {}, ValueError, "one-dimensional channels or"),
    (_cr, "cancel_echoes", (CH[:0], CH[:0], 1e5, [3], [1.0]), {}, ValueError, "empty channels"),
    (_cr, "cancel_echoes", (CH, CH, 1e5, [2.5], [1.0]), {}, ValueError, "echo lags are whole samples"),
    (_cr, "cancel_echoes", (CH, CH, 1e5, [64], [1.0]), {}, ValueError, "echo lag outside"),
    (_cr, "cancel_echoes", (CH, CH, 1e5, [3], [float("nan")]), {}, ValueError, "echo Dopplers must be finite"),
    (_cr, "cancel_echoes", (CH, CH, 1e5, [3, 4], [1.0]), {}, ValueError, "same length"),
    (_cr, "cancel_echoes", (np.ones((2, 64), np.complex64),) * 2 + (1e5, [[3]], [[1.0]]), {}, ValueError, "takes 2 lists"),
    (_cr, "cancel_echoes", (CH, CH, 1e5, [3], [1.0]), dict(reg=-1.0), ValueError, "reg = -1, not finite and >= 0"),
    (_cr, "cancel_echoes", (CH, CH, 1e5, list(range(33)), [1.0] * 33), {}, ValueError, "max_atoms = 33 outside 1 .. 32"),
]


def _id(case):
    return case[1] + "-" + ",".join(f"{k}={getattr(v, 'shape', v)}" for k, v in case[3].items())


@pytest.mark.parametrize("case", CASES, ids=[f"{i:02d}-{_id(c)}" for i, c in enumerate(CASES)])
def test_check_raises_before_a_device_is_touched(case, monkeypatch):
    from passiveradar_amd import _lib
    module, name, args, kw, exc, message = case
    touched = []

    def require_gpu():
        touched.append("require_gpu")
        raise RuntimeError("a device was asked for")

    def buffer_init(self, nbytes):
        touched.append("DeviceBuffer")
        raise RuntimeError("a device buffer was asked for")

    monkeypatch.setattr(_lib, "require_gpu", require_gpu)
    monkeypatch.setattr(_lib.DeviceBuffer, "__init__", buffer_init)
    monkeypatch.setattr(_lib, "torch_stream_ptr", lambda device=None: None)     # a stand-in tensor has no stream to ask for
    with pytest.raises(exc, match=message):
        getattr(module(), name)(*args, **kw)
    assert touched == []


def test_empty_inputs_touch_no_device(monkeypatch):
    """the shortcuts: no ends, no patches, no atoms"""
    from passiveradar_amd import _lib
    touched = []
    monkeypatch.setattr(_lib, "require_gpu", lambda: touched.append("require_gpu"))
    monkeypatch.setattr(_lib.DeviceBuffer, "__init__", lambda self, nbytes: touched.append("DeviceBuffer"))
    paths = _td().tbd_paths(B3, np.zeros((0, 2), np.int32), 4)
    assert paths.shape == (0, 4) and paths.dtype == np.int32
    pk = _td().refine_peaks(P3[:0], [], [], 1.0)
    assert pk.shape == (0,) and pk.dtype == _lib.PATCH_PEAK_DTYPE
    assert _cr().cancel_echoes(CH, CH, 1e5, [], []) is CH
    assert touched == []
