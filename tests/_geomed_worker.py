"""Worker of test_geomed_*: W gloo ranks aggregate three tensors with ``RobustRule("geomed").gather_combine_`` in
two buckets (the second one flattened from two tensors) and compare with ``combine`` on the whole gathered
stack, bit for bit.  With ``--device cuda`` the ranks share the card and the kernels of csrc/geomed.hip run;
the aggregate's digest is printed so that the test can compare the ranks."""
import hashlib
import sys

import torch
import torch.distributed as dist

from fedrec_with_pytorchdistributed_amd.parallel.robust import RobustRule

dist.init_process_group("gloo")
rank, W = dist.get_rank(), dist.get_world_size()
dev = torch.device(sys.argv[sys.argv.index("--device") + 1] if "--device" in sys.argv else "cpu")
g = torch.Generator().manual_seed(5)
base = torch.randn(3000 + 1500 + 2051, generator=g)
mine = base + 1e-2 * torch.randn(base.numel(), generator=torch.Generator().manual_seed(100 + rank))
rows = [torch.empty_like(mine) for _ in range(W)]
dist.all_gather(rows, mine)
want, wd = RobustRule("geomed").combine(torch.stack(rows).to(dev))
ts = [t.clone().to(dev) for t in mine.split([3000, 1500, 2051])]
rule = RobustRule("geomed")
dropped = rule.gather_combine_(ts, None, W, bucket_bytes=4 * 4000)  # [3000] | [1500, 2051]
got = torch.cat(ts).cpu()
ok = torch.equal(got.view(torch.int32), want.cpu().view(torch.int32)) and dropped.tolist() == wd.tolist() == [0] * W
ok = ok and rule.record(dropped, got.numel(), W)["agg_weight"] == [float(x) for x in rule.weights.cpu()]
print("GEOMED OK" if ok else "GEOMED FAIL", hashlib.sha256(got.numpy().tobytes()).hexdigest(), flush=True)
dist.destroy_process_group()
