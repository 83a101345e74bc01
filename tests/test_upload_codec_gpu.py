"""The star's upload codec on the device against the same codec on the host: the one bitwise contract that
lets a single codec serve the coordinator (host) and clients that combine among themselves (device).  The
kernels are held to it at the ``ops`` level; this holds the codec's plumbing around them -- contiguity, dtype
views, and the composed top-k + quantise residual update."""
import pytest
import torch

from test_upload_codec_cpu import FORMS, N, W, WEIGHTS, compress_all, make_codec, same

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("form", list(FORMS))
def test_device_and_host_give_the_same_blobs_residuals_and_aggregate(form):
    codec, _ = make_codec(form)
    theta_h, pays_h, res_h = compress_all(codec)
    theta_d, pays_d, res_d = compress_all(codec, "cuda")
    for c in range(W):
        blob = codec.pack(pays_d[c])
        assert blob.is_cuda and same(blob, codec.pack(pays_h[c]))
        if codec.uses_residual:
            assert res_d[c].is_cuda and same(res_d[c], res_h[c])
    new_h, _ = codec.combine(theta_h, pays_h, WEIGHTS)
    new_d, _ = codec.combine(theta_d, pays_d, WEIGHTS)
    assert new_d.is_cuda and new_d.numel() == N and same(new_d, new_h)
    if form != "dense":  # (the weights as a gather among the clients leaves them: on the device already)
        assert same(codec.combine(theta_d, pays_d, torch.tensor(WEIGHTS, device="cuda"))[0], new_h)
