"""GPU: _lib.call and _lib.workspace, the one call path from Python into the C ABI -- the device made current, ``_lib.STREAM`` replaced by
that device's current stream, a non-zero status raised under the symbol's name.  The first test substitutes a recording fake for the
library and launches no kernel; the second runs two real entry points on a side stream against the default stream."""
import pytest
import torch

from oai_analysis_2_amd import _lib, ops

pytestmark = pytest.mark.gpu


class FakeLib:
    """Records the arguments of two entry points that do nothing: one reports success, one status 7."""

    def __init__(self):
        self.calls = []
        self.bytes = 0

    def oai_fake_ok(self, *args):
        self.calls.append(args)
        return 0

    def oai_fake_seven(self, *args):
        self.calls.append(args)
        return 7

    def oai_fake_workspace_bytes(self, *size_args):
        self.calls.append(size_args)
        return self.bytes

    def oai_last_error(self):
        return b"seven was asked for"


def test_call_passes_the_current_stream_of_the_device_and_raises_on_status(monkeypatch):
    fake = FakeLib()
    monkeypatch.setattr(_lib, "_lib", fake)
    for name in ("oai_fake_ok", "oai_fake_seven"):
        monkeypatch.setitem(_lib.SIGNATURES, name, (_lib.C.c_int, []))
    s = torch.cuda.Stream(device=0)
    default = torch.cuda.default_stream(0).cuda_stream
    assert s.cuda_stream != default
    with torch.cuda.stream(s):
        _lib.call("oai_fake_ok", 1, _lib.STREAM, 2, device=0)
    assert fake.calls.pop() == (1, s.cuda_stream, 2)
    _lib.call("oai_fake_ok", 1, _lib.STREAM, 2, device=0)
    assert fake.calls.pop() == (1, default, 2)
    with pytest.raises(_lib.OaiError, match=r"^oai_fake_seven failed \(7\): seven was asked for"):
        _lib.call("oai_fake_seven", 1, _lib.STREAM, 2, device=0)
    assert fake.calls.pop() == (1, default, 2)
    for pad, want in ((False, 0), (True, 1)):
        ws = _lib.workspace("oai_fake", "cuda:0", 3, 4, pad=pad)
        assert fake.calls.pop() == (3, 4)
        assert ws.numel() == want and ws.dtype == torch.uint8 and ws.device == torch.device("cuda", 0)
    fake.bytes = 24
    assert _lib.workspace("oai_fake", "cuda:0", pad=True).numel() == 24


def test_real_entry_points_follow_a_side_stream():
    """ops.mask_overlap and ops.phi_jacobian queued under ``torch.cuda.stream(s)`` give the tensors of the default stream."""
    g = torch.Generator().manual_seed(5)
    a = torch.rand(8, generator=g).cuda()
    phi = torch.rand((3, 3, 4, 5), generator=g).cuda()
    want_counts, want_stats = ops.mask_overlap(a), ops.phi_jacobian(phi)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        counts, stats = ops.mask_overlap(a), ops.phi_jacobian(phi)
    s.synchronize()
    assert torch.equal(counts, want_counts) and torch.equal(stats, want_stats)
    assert int(want_counts[0]) == int((a > 0.5).sum()) and int(want_stats[0]) == 2 * 3 * 4
