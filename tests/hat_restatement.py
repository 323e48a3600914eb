"""Float64 torch restatement of the HAT (hybrid autoregressive transducer) lattices built by
tf_fast_rnnt.get_hat_logprobs_pruned / get_hat_logprobs_joint.  TEST INFRASTRUCTURE ONLY: nothing in the product package
imports this file.

For one joiner row x = logits[b,t,k,:] and blank = termination_symbol:

    log P(blank) = log sigmoid(x[blank])
    log P(c)     = log sigmoid(-x[blank]) + log_softmax over the non-blank columns of x, at c      (c != blank)

written directly with logsigmoid and a masked log_softmax (not through the identity with an ordinary softmax, so that the
tests can check that identity against this file).  The band is padded and rolled into full-size lattices as the ordinary
pruned builder does it (oracle/rnnt_oracle.py get_rnnt_logprobs_pruned); a symbol equal to blank gets px = -inf."""
from typing import Optional, Tuple

import torch

from tf_fast_rnnt.rnnt_loss import _check_type, _i64, _NEG_INF, fix_for_boundary
from torch_restatements import roll_by_shifts


def hat_log_probs(logits: torch.Tensor, blank: int) -> torch.Tensor:
    """[..., C] -> [..., C]: entry blank is log P(blank), every other entry c is log P(c)."""
    C = logits.shape[-1]
    is_blank = torch.zeros(C, dtype=torch.bool, device=logits.device)
    is_blank[blank] = True
    xb = logits[..., blank:blank + 1]
    nonblank = torch.log_softmax(logits.masked_fill(is_blank, _NEG_INF), dim=-1)
    return torch.where(is_blank, torch.nn.functional.logsigmoid(xb), nonblank + torch.nn.functional.logsigmoid(-xb))


def get_hat_logprobs_pruned_torch(
    logits: torch.Tensor,
    symbols: torch.Tensor,
    ranges: torch.Tensor,
    termination_symbol: int,
    boundary: Optional[torch.Tensor] = None,
    rnnt_type: str = "regular",
) -> Tuple[torch.Tensor, torch.Tensor]:
    """logits [B,T,r,C] -> px [B,S,T+1|T], py [B,S+1,T], in the dtype and on the device of logits."""
    _check_type(rnnt_type)
    B, T, r, C = logits.shape
    sym = _i64(symbols)
    S = sym.shape[1]
    rg = _i64(ranges)
    logp = hat_log_probs(logits, termination_symbol)                                  # [B,T,r,C]
    sym_ext = torch.cat((sym, torch.full((B, 1), termination_symbol, dtype=torch.int64, device=sym.device)), dim=1)
    pruned_sym = torch.gather(sym_ext.unsqueeze(1).expand(B, T, S + 1), 2, rg)        # [B,T,r]
    px = torch.gather(logp, 3, pruned_sym.unsqueeze(-1)).squeeze(-1)
    px = px.masked_fill(pruned_sym == termination_symbol, _NEG_INF)                   # blank is not a symbol
    pad = torch.full((B, T, S + 1 - r), _NEG_INF, dtype=logits.dtype, device=logits.device)
    px = roll_by_shifts(torch.cat((px, pad), dim=2), rg[:, :, 0])[:, :, :S].permute(0, 2, 1)   # [B,S,T]
    if rnnt_type == "regular":
        px = torch.cat((px, torch.full((B, S, 1), _NEG_INF, dtype=logits.dtype, device=logits.device)), dim=2)
    py = logp[..., termination_symbol]
    py = roll_by_shifts(torch.cat((py, pad), dim=2), rg[:, :, 0]).permute(0, 2, 1)            # [B,S+1,T]
    if rnnt_type == "regular":
        px = fix_for_boundary(px, boundary)
    elif rnnt_type == "constrained":
        px = px + py[:, 1:, :]
    return px.contiguous(), py.contiguous()


def get_hat_logprobs_joint_torch(logits, symbols, termination_symbol, boundary=None, rnnt_type="regular"):
    """logits [B,T,S+1,C]: the pruned form with identity ranges."""
    B, T, S1, _ = logits.shape
    ranges = torch.arange(S1, device=logits.device).expand(B, T, S1)
    return get_hat_logprobs_pruned_torch(logits, symbols, ranges, termination_symbol, boundary, rnnt_type)


def lattice_loss_torch(px: torch.Tensor, py: torch.Tensor, boundary, rnnt_type: str) -> torch.Tensor:
    """-log of the total path probability per utterance, as a float64 log-domain DP with autograd (the shape of the
    reference check in tests/test_gpu_pipeline.py).  boundary: int array [B,4]."""
    B = px.shape[0]
    out = []
    for b in range(B):
        sb, tb, se, te = [int(v) for v in boundary[b]]
        p = {}
        for s in range(sb, se + 1):
            for t in range(tb, te + 1):
                if s == sb and t == tb:
                    p[(s, t)] = px.new_zeros(())
                    continue
                terms = []
                if s > sb:
                    tt = t if rnnt_type == "regular" else t - 1
                    if tt >= tb and (s - 1, tt) in p and torch.isfinite(px[b, s - 1, tt]):
                        terms.append(p[(s - 1, tt)] + px[b, s - 1, tt])
                if t > tb and (s, t - 1) in p:
                    terms.append(p[(s, t - 1)] + py[b, s, t - 1])
                if terms:
                    p[(s, t)] = torch.logsumexp(torch.stack(terms), 0)
        out.append(-p[(se, te)] if (se, te) in p else px.new_full((), float("inf")))
    return torch.stack(out)
