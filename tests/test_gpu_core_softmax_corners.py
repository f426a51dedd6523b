"""The self-attention core at its online-softmax corners (run with -m gpu on an MI355X): attention_kernel, attention16s_kernel,
attention16g_kernel and attention_f32_kernel under every launch plan -- single, host tail, device plan, split_all -- and so
the three combine kernels on records whose maxima lie 12 to several hundred log2 units apart, in fp16 and bf16 (fp32 for the
f32 family).  One test per (family configuration, plan, dtype); each is ONE raw library call through run_case of
test_gpu_attention_plans.py -- its operand windows, garbage, canaries, selection and workspace checks -- with the operands
of tests/core_softmax_corners.py in the live windows: every (source sample, head) pair of the call carries one scenario
(a spike that comes late, staircases above and just below the deferred-rescale threshold, a dominant first / last key, rows
far below zero, wide scores, a jump that only a folded key's multiplicity makes) or stays the unplanted control, and the
planted rows and keys sit where the plan cuts the work: whole and split items of every tier, the partial last wave, row
count - 1; the tiles on both sides of a piece boundary, the last full tile and the ragged one.
test_core_softmax_corners_host.py proves on the host that every launch here reaches the branches it is built for and
that a dropped alpha, a combine without its weights or a stale shift would move the planted rows by ten bars and more.

Reference: the plain float64 softmax on the same rounded operands (folded keys: the multiplicity as a weight, which is the
duplicated sequence), on the planted rows, on the first / last / two random rows of every live query block and on row
count - 1.  Every compared row of every slot counts.  Bars as in run_case: 1e-3 (fp16) / 8e-3 (bf16) of max(1, |ref|max)
over the launch, BAR of test_gpu_fp32_attention.py of |ref|max for fp32.

The one widening.  The d % 16 != 0 heads (d = 8, 40: attention_kernel's BIAS path, attention16s, attention16g) pre-scale
the query in fp32 and round it to the operand type once more (attention.hip:170-175), |logit| 2^-12 per score in fp16 and
2^-9 in bf16.  On N(0, 1) operands that is inside the bar.  The wide_range slots of those heads (|logit| to 50 log2 units
between keys of comparable weight) are the ones where it is not -- 0.9 to 2.6 plain bars measured, printed next to each
ratio -- and their bar gets an added term per element: 2 x |float64 reference with the query pre-scaled and rounded that
way - plain reference|, from the operands alone (Launch.prescaled_term).  The all_very_negative slots stay inside the
plain bar (0.42 at most) and carry no term, nor does any other slot, any d % 16 == 0 head or the fp32 family.

Exact rows: where one key leads every other by 150 log2 units and more (first_key_dominant, last_key_dominant), every
other exp2 is 0 and under a split plan every other piece's weight is 0.  In the 16-bit families the P that meets V is
rounded to the operand type -- exactly 1 on that key -- and the quotient is rounded to it once more: every row of the slot
is that key's v row bit for bit.  attention_f32_kernel keeps P in fp32 and takes its exponent against the ROUNDED scaled
maximum, fmaf(s, c, -fl(s_max c)) (attention_f32.hip:285, 307): on the leading key that is the rounding residue of the
product, up to 2^-17 at 200 log2 units, not 0, so p = 1 + O(1e-5) there and no float64 model says "exactly 1".  What its
arithmetic does give is out = fl(fl(p v) * rcp(p)): two roundings of 2^-24 and a reciprocal good to one ulp, so the f32
rows are held to |out - v| <= 2^-22 |v| per element (ONE_KEY_F32) instead of to the bits; measured: 2^-24.  Under the device plan the call is run once more with other v rows at the planted keys: the planted rows
follow the float64 model, the control head keeps its bits.

Every case prints its slots' worst error over the bar (-s); profiles/core_softmax_corners.txt holds one run."""
import numpy as np
import pytest
import torch

import core_softmax_corners as CSC
from test_gpu_attention_plans import DEV, cus, run_case

pytestmark = pytest.mark.gpu
ONE_KEY_F32 = 2.0 ** -22                                      # see "Exact rows" above


@pytest.fixture(scope="module")
def L():
    from vidtome_amd import _lib
    _lib.lib()
    return _lib


class Hook:
    """run_case's operand hook for one Launch (see run_case)."""

    def __init__(self, launch):
        self.L = launch
        self.plain = {}                       # slots with the pre-scaled term: their worst error over the plain bar

    def operands(self, sel, q, k, v, rows, cnt, kc):
        Ln = self.L
        assert (sel.split, sel.header, sel.nqb) == (Ln.sel.split, Ln.sel.header, Ln.sel.nqb), "the host's plan is not the call's"
        assert list(cnt) == Ln.cnt and list(kc) == Ln.kc
        q[:Ln.src, :Ln.Mq] = Ln.q.to(DEV)
        k[:Ln.src, :Ln.Mk] = Ln.k.to(DEV)
        v[:] = Ln.v.to(DEV)
        for b in range(Ln.B):
            for head in range(CSC.H):
                rows[b] |= set(Ln.slot_of(b, head).rows)
            assert max(rows[b]) < cnt[b]

    def _errors(self, out, rows, v=None, only=None):
        """Per (output sample, slot): (error / bar per element).max(), with the bar of the whole launch."""
        Ln, d = self.L, self.L.d
        refs, scale_max = {}, 0.0
        for b in range(Ln.B):
            R = sorted(rows[b])
            got = out[b, torch.tensor(R, device=DEV)].double().cpu().numpy()
            for head in range(CSC.H):
                s = Ln.slot_of(b, head)
                if only is not None and not only(s):
                    continue
                keep = set(s.rows)
                RR = R if only is None else [r for r in R if r in keep]
                g = got[[i for i, r in enumerate(R) if r in keep]] if only is not None else got
                ref = Ln.reference(b, s, RR, v=v)
                refs[(b, head)] = (s, RR, ref, g[:, head * d:(head + 1) * d])
                scale_max = max(scale_max, float(np.abs(ref).max()))
        bar = Ln.bar(scale_max)
        worst = {}
        for (b, head), (s, RR, ref, g) in refs.items():
            assert np.isfinite(g).all(), (b, head, s.name, "non-finite output")
            allowed = bar
            if Ln.carries_prescaled_term(s):
                allowed = bar + Ln.prescaled_term(b, s, RR, ref)
                self.plain[s.name] = max(self.plain.get(s.name, 0.0), float(np.abs(g - ref).max()) / bar)
            worst[(b, head, s.name)] = float((np.abs(g - ref) / allowed).max())
        return worst, bar, scale_max

    def compare(self, sel, launch, out, vt, rows, cnt, kc):
        Ln, d = self.L, self.L.d
        worst, bar, scale_max = self._errors(out, rows)
        by_name = {}
        for (b, head, name), w in worst.items():
            by_name[name] = max(by_name.get(name, 0.0), w)
        line = " ".join(f"{n}={w:.3f}" + (f"(plain bar: {self.plain[n]:.3f})" if n in self.plain else "")
                        for n, w in sorted(by_name.items()))
        print(f"core {CSC.case_id((Ln.cfg.name, Ln.plan, Ln.dtype))} {sel.kind}/{sel.plan}/{sel.combine} bar={bar:.3e} "
              f"scale={scale_max:.3g} worst/bar: {line}")
        if Ln.dtype == torch.float32:
            assert scale_max > 0.05, "the comparison should not be about zeros"
        missed = {k_: w for k_, w in worst.items() if not w < 1.0}
        assert not missed, ("(sample, head, scenario): worst error over the bar", missed)
        # rows that are one key's v row, bit for bit
        for b in range(Ln.B):
            for head in range(CSC.H):
                s = Ln.slot_of(b, head)
                if s.one_key is not None:
                    sl = slice(head * d, (head + 1) * d)
                    want = vt[b, sl, s.one_key][None, :].expand(cnt[b], -1)
                    if Ln.dtype == torch.float32:
                        off = float(((out[b, :cnt[b], sl] - want).abs() / want.abs()).max())
                        assert off <= ONE_KEY_F32, (b, head, s.name, "not the key's v row to 2^-22", off)
                    else:
                        assert torch.equal(out[b, :cnt[b], sl], want), (b, head, s.name, "not the key's v row bit for bit")
        if Ln.plan != CSC.SENSITIVITY_PLAN:
            return
        # the planted keys' v rows changed: the planted rows follow the model, the control head keeps its bits
        g = torch.Generator().manual_seed(11)
        v2 = Ln.v.clone()
        for b in range(Ln.B):
            for head in range(CSC.H):
                s = Ln.slot_of(b, head)
                if s.keys:
                    sl = slice(head * d, (head + 1) * d)
                    v2[b, s.keys, sl] = (torch.randn(len(s.keys), d, generator=g) + 3.0).to(Ln.dtype)
                    vt[b, sl][:, s.keys] = v2[b, s.keys, sl].t().to(DEV)
        out2 = launch()
        moved, bar2, _ = self._errors(out2, rows, v=v2, only=lambda s: bool(s.keys))
        missed = {k_: w for k_, w in moved.items() if not w < 1.0}
        assert not missed, ("planted rows do not follow the changed v rows", missed)
        for b in range(Ln.B):
            for head in range(CSC.H):
                s = Ln.slot_of(b, head)
                sl = slice(head * d, (head + 1) * d)
                if s.name == CSC.CONTROL:           # (bit patterns: the rows of dead blocks hold NaN canaries)
                    bits = torch.int32 if Ln.dtype == torch.float32 else torch.int16
                    assert torch.equal(out2.view(bits)[b, :, sl], out.view(bits)[b, :, sl]), (b, head, "the control head changed")
                elif s.keys:
                    R = [r for r in s.rows if r < cnt[b]]
                    step = np.abs(Ln.reference(b, s, R, v=v2) - Ln.reference(b, s, R)).max(1)
                    assert float(step.min()) > 10 * bar2, (b, head, s.name, "the changed v rows do not reach the planted rows")
        print(f"core {CSC.case_id((Ln.cfg.name, Ln.plan, Ln.dtype))} changed v rows: worst/bar "
              f"{max(moved.values()):.3f}, control head unchanged")


@pytest.mark.parametrize("case", CSC.gpu_cases(), ids=CSC.case_id)
def test_core_corner(L, oracle, case):
    Ln = CSC.build(*case, cus())
    a = dict(Ln.args)
    a["mult"] = Ln.mult
    sel = run_case(L, oracle, dtype=case[2], hook=Hook(Ln), **a)
    assert (sel.kind, sel.plan, sel.combine) == a["expect"]
