"""Sparsified uploads through the star drivers with the clients on the GPU: two client processes share
the card (``FEDREC_SHARE_GPU=1``) over a gloo data plane, as the other multi-rank GPU tests do.  The
clients compress with the ``topk_delta`` kernel and combine among themselves with the ``combine``
kernel; the test recomputes the round from their dumped parameters with the host oracles, and the
coordinator's global model must hold the same bits."""
import pytest

from test_sparse_star_cpu import W, assert_global_is, expected_round0, star

SHARE = {"FEDREC_CPU_ONLY": "0", "FEDREC_SHARE_GPU": "1", "FEDREC_DATA_BACKEND": "gloo", "FEDREC_QUIET": "1"}
FLAGS = ["--data_dir=synthetic:tiny", "--round_timeout_s=300", "--collective_timeout_s=300"]


@pytest.mark.gpu
def test_one_sparse_round_on_the_device_is_the_host_oracles_bit_for_bit(tmp_path, dev):
    d = tmp_path / "gpu"
    (rec,) = star(d, 1, [*FLAGS, "--upload_topk=0.05"], "allreduce", SHARE, timeout=400)
    want, flat, n, k = expected_round0(d, FLAGS, 0.05)
    assert_global_is(d, want, flat)
    assert rec["clients_accepted"] == W and rec["upload_bytes"] < rec["dense_bytes"] // 4
