"""The backward's cached partial-sum scratch (_base._accum) and hipGraph capture: every capture runs on torch's capture
stream, whose handle torch's stream pool also hands to eager code, so a capture must neither take a buffer from the cache nor
leave one there -- or graphs replayed side by side on different streams (FramePipeline) share their partial sums."""
import pytest
import torch

from skelsplat_amd import _base

pytestmark = pytest.mark.gpu


def test_a_capture_never_takes_its_scratch_from_the_cache(device):
    V, P, C = 3, 5, 7                   # (a shape nothing else uses)
    seen = {}

    def capture():
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            handle = torch.cuda.current_stream(device).cuda_stream
            buf = _base._accum(device, handle, V, P, C)
            buf.zero_()
        return graph, handle, buf

    g1, handle, first = capture()
    key = (device.index, handle, V, P, C)
    assert key not in _base._accum_cache
    try:
        eager = _base._accum(device, handle, V, P, C)           # eager code on a stream with the capture stream's handle
        assert _base._accum_cache[key] is eager and _base._accum(device, handle, V, P, C) is eager
        g2, handle2, second = capture()
        assert handle2 == handle
        assert second.data_ptr() != eager.data_ptr() and second.data_ptr() != first.data_ptr()
        assert _base._accum_cache[key] is eager
    finally:
        _base._accum_cache.pop(key, None)
