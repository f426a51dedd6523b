"""CPU test: the oracle's restatement of the merge closures' reduce modes (oracle.scatter_reduce / the `merge` closure's
``mode=`` and ``round_to=``) against the operation it restates, torch's CPU ``scatter_reduce(..., include_self=True)``, bit
for bit -- at destination rows with 1 to 4099 members, on both sides of the largest member count that fp16 (2048) and
bf16 (256) represent exactly.  tests/golden/modes.npz stops at 8 members per row, where "divide by the count" and "divide
by the count rounded to the tensors' dtype" are the same rule; torch applies the second."""
import numpy as np
import pytest
import torch

from helpers import MEMBER_COUNTS, REDUCE_MODES, interleaved_destinations, reduce_tokens, same_bits, scatter_reduce_reference

DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
ROUNDERS = {"fp32": None, "fp16": lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).half().numpy(),
            "bf16": lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).bfloat16().float().numpy()}
C = 16


@pytest.mark.parametrize("mode", REDUCE_MODES)
@pytest.mark.parametrize("name", list(DTYPES))
def test_oracle_merge_modes_vs_torch_scatter_reduce(oracle, name, mode):
    dt, counts = DTYPES[name], MEMBER_COUNTS[name]
    dst_idx = interleaved_destinations(counts, seed=len(counts))
    Nd, r = len(counts), dst_idx.shape[1]
    assert r == sum(counts) - Nd and max(counts) > {"fp32": 2500, "fp16": 2048, "bf16": 256}[name]
    x = reduce_tokens((1, r + Nd, C), dt, seed=17, mode=mode)
    # src tokens at rows [Nd, Nd + r) taken in a scrambled src_idx order, dst tokens at rows [0, Nd)
    src_idx = torch.randperm(r, generator=torch.Generator().manual_seed(3))[None]
    a_idx, b_idx = np.arange(Nd, Nd + r), np.arange(Nd)
    # the row of two members: every pairing of +0 and -0, self first (amax / amin keep the zero that came first)
    assert counts[1] == 2
    pair = int((dst_idx[0] == 1).nonzero()[0])
    x[0, 1, :4] = torch.tensor([0.0, 0.0, -0.0, -0.0]).to(dt)
    x[0, Nd + int(src_idx[0, pair]), :4] = torch.tensor([0.0, -0.0, 0.0, -0.0]).to(dt)
    want = scatter_reduce_reference(x, torch.from_numpy(a_idx)[src_idx], torch.from_numpy(b_idx)[None], dst_idx, mode)
    merge, _ = oracle._closures(a_idx, b_idx, np.zeros((1, 0), np.int64), src_idx.numpy(), dst_idx.numpy().astype(np.int64), r + Nd)
    got = merge(x.float().numpy(), mode=mode, round_to=ROUNDERS[name])
    got = torch.from_numpy(np.ascontiguousarray(got, dtype=np.float32)).to(dt)      # (already rounded: exact)
    same = same_bits(got, want)
    bad = {counts[j]: int((~same[0, j]).sum()) for j in range(Nd) if not same[0, j].all()}
    assert not bad, f"{name} {mode}: differing channels (of {C}) by member count: {bad}"
