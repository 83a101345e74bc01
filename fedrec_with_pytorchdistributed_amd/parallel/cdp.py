"""Client-level differential privacy on the star round update (``cfg.cdp``): DP-FedAvg (McMahan, Ramage,
Talwar, Zhang 2018) with the noise added by the clients themselves (distributed DP).

Each client clips its round delta ``local - theta_g`` to an L2 norm ``C`` and adds Gaussian noise of standard
deviation ``z C / sqrt(W)``: ``W`` such shares sum to variance ``(z C)^2`` on the sum, whose sensitivity to one
client is ``C``.  Both happen before the upload, so the rule composes with secure aggregation (nobody has to see
an update to bound it) and the coordinator is not trusted for privacy; the server-side step is post-processing.
The arithmetic is :func:`ops.dp_delta_sqnorm` and :func:`ops.dp_clip_noise` -- csrc/dp_clip.hip on a device
tensor, the torch oracles on the host.  The unit of privacy is a client's whole round, not one occurrence in
one step as under ``cfg.dp``.

The coordinator accounts every aggregated round with the RDP accountant at sample rate 1: a round that took
``A`` of ``W`` uploads carries ``A`` shares, so it is accounted at ``z sqrt(A / W)``.  The unclipped norm and the
``clipped`` flag of a client are private: they stay in :attr:`ClientDP.last` for the client's own log.
"""
from __future__ import annotations

import math
import secrets
from typing import Dict, List, Optional

import torch

from .. import ops
from ..ops import reference as ref
from ..privacy import rdp


class ClientDP:
    def __init__(self, clip: float = 0.0, noise_multiplier: float = 0.0, delta: float = 1e-5, seed: int = 0,
                 clients: int = 1):
        if not (clip >= 0.0 and math.isfinite(clip)):
            raise ValueError(f"cdp.clip={clip}: must be >= 0 and finite (0 is off)")
        if not (noise_multiplier >= 0.0 and math.isfinite(noise_multiplier)):
            raise ValueError(f"cdp.noise_multiplier={noise_multiplier}: must be >= 0 and finite")
        if not 0.0 < delta < 1.0:
            raise ValueError(f"cdp.delta={delta}: must lie in (0, 1)")
        self.clip, self.z, self.delta = float(clip), float(noise_multiplier), float(delta)
        self.clients = max(1, int(clients))
        # seed 0: a key from OS entropy, held by this object alone (never logged, never sent)
        self._key = int(seed) if seed else secrets.randbits(63) | 1
        self.accountant = rdp.RDPAccountant()
        self.last: Optional[Dict] = None  # this client's own (norm, scale, clipped) of the last round: private

    @classmethod
    def from_cfg(cls, cfg, driver: str = "fedavg_star", clients: int = 1) -> "ClientDP":
        """The rule of ``cfg``; an active one is rejected where its guarantee would not hold (``driver``: the
        federation driver that asks), before the first round."""
        c = cfg.cdp
        if not c.clip:
            return cls()
        if driver != "fedavg_star":
            raise ValueError(f"cdp.clip={c.clip} is not available with mode={driver}: client-level DP bounds a star "
                             "client's round delta (use fedavg_star)")
        if cfg.robust_agg != "none":
            raise ValueError(f"cdp.clip={c.clip} cannot be combined with robust_agg={cfg.robust_agg}: the rule re-weights "
                             "the clients, and the sensitivity bound is for the plain sum")
        if cfg.weighted_fedavg:
            raise ValueError(f"cdp.clip={c.clip} cannot be combined with weighted_fedavg=1: a weighted client moves "
                             "the sum by more than its clip")
        if cfg.upload_topk:
            raise ValueError(f"cdp.clip={c.clip} cannot be combined with upload_topk={cfg.upload_topk}: the "
                             "error-feedback residual is unprivatised state")
        if cfg.upload_bits:
            raise ValueError(f"cdp.clip={c.clip} cannot be combined with upload_bits={cfg.upload_bits}: the "
                             "error-feedback residual is unprivatised state")
        if cfg.upload_sign:
            raise ValueError(f"cdp.clip={c.clip} cannot be combined with upload_sign={cfg.upload_sign}: the "
                             "error-feedback residual is unprivatised state")
        if cfg.upload_rank:
            raise ValueError(f"cdp.clip={c.clip} cannot be combined with upload_rank={cfg.upload_rank}: the "
                             "error-feedback residual is unprivatised state")
        z = c.noise_multiplier
        if z is None:
            if not c.epsilon > 0:
                raise ValueError(f"cdp.clip={c.clip} needs cdp.noise_multiplier (0 = clip only) or cdp.epsilon > 0")
            z = rdp.get_noise_multiplier(c.epsilon, c.delta, sample_rate=1.0, steps=max(1, int(cfg.global_rounds)))
        return cls(c.clip, z, c.delta, c.seed, clients)

    @property
    def active(self) -> bool:
        return self.clip > 0.0

    def std_for(self, W: int) -> float:
        """One client's noise scale: ``W`` shares of this variance sum to ``(z C)^2``."""
        return self.z * self.clip / math.sqrt(max(1, int(W)))

    def privatize(self, up: torch.Tensor, theta_g: torch.Tensor, client: int, round_idx: int) -> torch.Tensor:
        """``theta_g + clip(up - theta_g) + noise``: two ops, nothing read back for the arithmetic."""
        local, base = up.float().contiguous(), theta_g.float().contiguous()
        state = ops.dp_delta_sqnorm(local, base)
        out = ops.dp_clip_noise(local, base, state, self.clip, self.std_for(self.clients), self._key,
                                (int(client) << 32) | int(round_idx))
        sq, s, clipped = ref.dp_state_fields(state)
        self.last = {"delta_norm": math.sqrt(sq) if sq >= 0 else float("nan"), "scale": s, "clipped": clipped}
        return out

    def record(self, accepted: int, W: int, spent: bool = True) -> Dict:
        """The keys a round record gains; ``spent``: the round's aggregate went into the global model (one that
        was rejected released nothing and spends nothing)."""
        z_eff = self.z * math.sqrt(max(0, int(accepted)) / max(1, int(W)))
        if spent:
            self.accountant.step(z_eff, 1.0)
        eps = self.accountant.get_epsilon(self.delta) if self.accountant.history else 0.0
        return {"cdp_clip": self.clip, "cdp_noise_multiplier": self.z, "cdp_noise_effective": z_eff,
                "cdp_epsilon": float(eps), "cdp_delta": self.delta}

    def state(self) -> Optional[Dict]:
        """The accountant's history, for the coordinator's snapshot."""
        return {"cdp_history": [[float(s), float(q), int(n)] for s, q, n in self.accountant.history]} if self.active else None

    def load(self, st: Optional[Dict]) -> None:
        hist: List = (st or {}).get("cdp_history") or []
        self.accountant.history = [(float(s), float(q), int(n)) for s, q, n in hist]
