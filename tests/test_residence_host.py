"""passiveradar_amd/residence.py on the host: which side a call gets, when the host side first asks for a device, and where
its buffers come from.  _lib.require_gpu, _lib.DeviceBuffer and the two library calls of an upload are recording stubs; no
GPU is needed."""
import ctypes

import numpy as np
import pytest


class FakeDeviceTensor:
    """what _lib.is_device_tensor takes for a device tensor"""
    is_cuda = True
    device = "cuda:0"

    def data_ptr(self):
        return 0


class StubBuffer:
    made = []

    def __init__(self, nbytes):
        self.nbytes, self.ptr = int(nbytes), 4096 * (len(StubBuffer.made) + 1)
        StubBuffer.made.append(self)

    def free(self):
        pass


class StubLib:
    """prc_memcpy_h2d keeps the bytes by destination; prc_stream_sync counts"""

    def __init__(self):
        self.uploaded, self.syncs = {}, 0

    def prc_memcpy_h2d(self, dst, src, nbytes, stream):
        assert stream is None
        self.uploaded[dst] = ctypes.string_at(src, nbytes)
        return 0

    def prc_stream_sync(self, stream):
        assert stream is None
        self.syncs += 1
        return 0


@pytest.fixture
def stubs(monkeypatch):
    from passiveradar_amd import _lib, engine, residence
    asked = []
    StubBuffer.made = []
    stub_lib = StubLib()
    monkeypatch.setattr(residence, "lib", lambda: stub_lib)
    monkeypatch.setattr(StubBuffer, "lib", stub_lib, raising=False)
    monkeypatch.setattr(_lib, "require_gpu", lambda: asked.append("require_gpu"))
    monkeypatch.setattr(_lib, "DeviceBuffer", StubBuffer)
    monkeypatch.setattr(_lib, "current_device", lambda: 0)
    monkeypatch.setattr(engine._tls, "staging", {}, raising=False)          # this thread's pool: empty, and put back after
    return asked


def test_of_picks_the_side_from_the_first_argument(monkeypatch):
    from passiveradar_amd import _lib, residence
    made = []
    monkeypatch.setattr(residence, "TorchSide", lambda device: made.append(device) or "torch side")
    assert residence.of(FakeDeviceTensor()) == "torch side" and made == ["cuda:0"]
    assert residence.of(FakeDeviceTensor(), None, FakeDeviceTensor()) == "torch side"
    for host in (np.ones(3), [1.0, 2.0], 5):
        side = residence.of(host, None, np.ones(2))
        assert isinstance(side, residence.HostSide) and side.pooled and not side.torch and side.stream is None
    assert not residence.of(np.ones(3), pooled=False).pooled
    assert not _lib.is_device_tensor(np.ones(3))


def test_a_mix_raises_with_the_callers_message(monkeypatch):
    from passiveradar_amd import residence
    monkeypatch.setattr(residence, "TorchSide", lambda device: pytest.fail("a side was made of a mix"))
    said = "stat and weight are both NumPy arrays or both device tensors"
    with pytest.raises(ValueError, match=said):
        residence.of(np.ones(3), FakeDeviceTensor(), mixed=said)
    with pytest.raises(ValueError, match=said):
        residence.of(FakeDeviceTensor(), None, np.ones(3), mixed=said)


@pytest.mark.parametrize("pooled", [True, False])
@pytest.mark.parametrize("first", ["put", "empty", "scratch"])
def test_host_side_asks_for_a_device_on_first_use_only(stubs, pooled, first):
    from passiveradar_amd import residence
    side = residence.HostSide(pooled)
    with side.device():
        pass
    assert side.scratch("ws", 0) is None
    assert stubs == [] and StubBuffer.made == []
    calls = {"put": lambda: side.put("x", [1, 2, 3], np.float32), "empty": lambda: side.empty("o", (2, 3), np.float64),
             "scratch": lambda: side.scratch("ws", 7)}
    h = calls[first]()
    assert stubs == ["require_gpu"] and h.nbytes == {"put": 12, "empty": 48, "scratch": 7}[first] and h.ptr
    for name in ("put", "empty", "scratch"):
        calls[name]()
    assert stubs == ["require_gpu"]
    assert side.scratch("ws", 0) is None


def test_put_uploads_the_contiguous_cast(stubs):
    from passiveradar_amd import residence
    x = np.arange(12, dtype=np.float64).reshape(3, 4)[:, ::2]
    h = residence.HostSide().put("x", x, np.float32)
    assert h.lib.uploaded == {h.ptr: np.ascontiguousarray(x, dtype=np.float32).tobytes()} and h.lib.syncs == 1


def test_pooled_buffers_come_from_staging_by_name(stubs):
    from passiveradar_amd import engine, residence
    side = residence.HostSide(pooled=True)
    a = side.scratch("cfar_ws", 100)
    assert engine.staging().bufs == {"cfar_ws": a}
    assert side.scratch("cfar_ws", 100) is a and side.empty("cfar_ws", (25,), np.float32) is a          # not larger: reused
    assert residence.HostSide(pooled=True).scratch("cfar_ws", 64) is a                                   # the pool outlives a side
    b = side.scratch("cfar_ws", 101)                                                                     # grow-only
    assert b is not a and b.nbytes == 101 and engine.staging().bufs == {"cfar_ws": b}
    c = side.put("cfar_x", np.ones(4, np.float32), np.float32)
    assert set(engine.staging().bufs) == {"cfar_ws", "cfar_x"} and c is not b


def test_fresh_buffers_are_distinct_and_held_by_the_side(stubs):
    from passiveradar_amd import engine, residence
    side = residence.HostSide(pooled=False)
    a, b, c = side.scratch("a", 16), side.scratch("b", 16), side.scratch("a", 16)
    assert len({id(a), id(b), id(c)}) == 3 and len(StubBuffer.made) == 3
    assert side._bufs.bufs == {"a": c, "b": b}                         # the latest of each name, until the side dies
    assert engine.staging().bufs == {}
