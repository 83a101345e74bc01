"""Block-quantized uploads through the star drivers with the clients on the GPU: two client processes
share the card (``FEDREC_SHARE_GPU=1``) over a gloo data plane, as the other multi-rank GPU tests do.  The
clients compress with the ``quantize_delta`` kernel and combine among themselves with the
``dequant_combine`` kernel; the test recomputes the round from their dumped parameters with the host
oracles -- which is also what the coordinator's host aggregate under ``upload`` computes -- and the
coordinator's global model must hold the same bits."""
import pytest

from test_quant_star_cpu import W, assert_global_is, expected_round0, star

SHARE = {"FEDREC_CPU_ONLY": "0", "FEDREC_SHARE_GPU": "1", "FEDREC_DATA_BACKEND": "gloo", "FEDREC_QUIET": "1"}
FLAGS = ["--data_dir=synthetic:tiny", "--round_timeout_s=300", "--collective_timeout_s=300"]


@pytest.mark.gpu
@pytest.mark.parametrize("extra,bits,fraction", [(["--upload_bits=8"], 8, 0.0),
                                                 (["--upload_bits=4", "--upload_topk=0.05"], 4, 0.05)])
def test_one_quantized_round_on_the_device_is_the_host_oracles_bit_for_bit(tmp_path, dev, extra, bits, fraction):
    d = tmp_path / "gpu"
    (rec,) = star(d, 1, [*FLAGS, *extra], "allreduce", SHARE, timeout=400)
    want, flat, n = expected_round0(d, FLAGS, bits, fraction)
    assert_global_is(d, want, flat)
    assert rec["clients_accepted"] == W and rec["upload_bits"] == bits and rec["upload_bytes"] < 0.27 * rec["dense_bytes"]
