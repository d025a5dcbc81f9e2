"""The actor step chain (csrc/actor.hip: k_act_qlin, k_act_vision,
k_act_convlstm, k_act_attn, k_act_ans0, k_act_ans2, k_act_lstmcell,
k_act_lstmcell_core behind aaa_actor_step / aaa_actor_step_core), each stage
held against fp64 evaluated on the operands the chain itself stored, element by
element: the stages' hand-offs come out of the workspace
(aaa_actor_workspace_region), the references and the bounds from
tests/actor_ref.py, whose docstring derives every constant from the kernels'
chain lengths.  tests/test_actor_emulation.py shows on the CPU that a correct
float32 kernel fits those bounds and that each seeded mistake breaks one.

Per case (actor_ref.CASES: P = 1, 4, 64, 121, 540, 1024, 1056, 2048 -- one
position, under one chunk, exact tiles and chunks, the workload, non-square,
nch = 64, 66 and 128 -- on both chains, B in {1, 4, 5, 16}, A in {1, 3, 17, 18,
256}, nq in {4, 8}, uint8 and non-integer fp32 frames, prev_reward /
prev_action given and NULL): two chained steps on one workspace from a
non-zero state, every region and output poisoned with a finite value before
each call; the second step then again from the same inputs, with attn / gates
/ actions / query NULL, and with the other of in-place / h_out, c_out: every
other output and region bit for bit the same.  The draw is aaa_sample_actions
on the chain's own logits bit for bit and the oracle's draw action for action.

Measured worst err / bound per stage and the expf term (MI355X): DESIGN.md
"Actor chain: accuracy on its own operands".
"""
import numpy as np
import pytest
import torch

import actor_ref as R
from helpers import detinit
from oracle import ref_cpu

import attention
from aaa_amd.policy import sample_actions

pytestmark = pytest.mark.gpu

SEED = 77
REGIONS = ("X", "HS", "HID1", "AO", "LH", "LOGITS", "ANSWER")
CORE_REGIONS = ("QT", "Q1", "Q2")


class _Chain:
    def __init__(self, cuda, c):
        from aaa_amd.runtime import ActorRunner
        H, W, B, nq, A, core, u8, prev, oop = c
        self.c, self.g, self.dev = c, R.geom(c), cuda
        raw, _ = R.params(nq, A)
        self.ar = ar = ActorRunner(B, H, W, nq, A, cuda, frames_u8=u8, stateful_core=core)
        assert (ar.h, ar.w) == (self.g["h"], self.g["w"])
        agent = attention.Agent(A, num_queries=nq, grid=(ar.h, ar.w), stateful_core=core)
        detinit.load_into(agent, raw)
        self.flat = torch.cat([p.detach().reshape(-1) for p in agent.parameters()]).to(cuda)
        assert self.flat.numel() == ar.n_params
        self.packed = ar.new_packed()
        ar.pack(self.flat, self.packed)
        self.S = agent.spatial.S.to(cuda).contiguous()
        self.ws = ar.new_workspace()
        self.ws.view(torch.float32).fill_(R.POISON)   # counters included: the vision launch zeroes them
        self.names = REGIONS + (CORE_REGIONS if core else ())

    def step(self, st, step, counter, oop, opt=True):
        """One step from the host state ``st`` on inputs(c, step).  Returns the run dict actor_ref.check takes
        (host tensors), plus "regions" and the draw's outputs."""
        H, W, B, nq, A, core, u8, prev, _ = self.c
        g, ar, dev = self.g, self.ar, self.dev
        fr, pr, pa = R.inputs(self.c, step)
        shp = ar.state_shape()
        d = lambda t: None if t is None else t.to(dev)                               # noqa: E731
        full = lambda *s, dt=torch.float32: torch.full(s, R.POISON if dt.is_floating_point else -7,   # noqa: E731
                                                       dtype=dt, device=dev)
        h, cc = st["h"].reshape(shp).to(dev), st["c"].reshape(shp).to(dev)
        out = dict(logits=full(B, A), values=full(B, A), attn=full(B, ar.h, ar.w, nq) if opt else None,
                   gates=full(B, ar.h, ar.w, 512) if opt else None,
                   actions=full(B, dt=torch.int32) if opt else None, logp=full(B) if opt else None,
                   dlogp=full(B, A) if opt else None, h_out=full(*shp) if oop else None,
                   c_out=full(*shp) if oop else None)
        kw = {}
        if core:
            kw = dict(core_h=st["core_h"].to(dev), core_c=st["core_c"].to(dev),
                      core_h_out=full(B, 256) if oop else None, core_c_out=full(B, 256) if oop else None,
                      query=full(B, nq, 72) if opt else None)
        ctr = torch.tensor([counter], dtype=torch.int64, device=dev)
        for name in self.names:
            ar.region(name, self.ws).fill_(R.POISON)
        ar.step(self.flat, self.packed, self.S, d(fr), self.ws, h, cc, out["logits"], out["values"],
                attn=out["attn"], prev_reward=d(pr), prev_action=d(pa), seed=SEED, counter=ctr,
                actions=out["actions"], logp=out["logp"], dlogp=out["dlogp"], gates=out["gates"],
                h_out=out["h_out"], c_out=out["c_out"], **kw)
        torch.cuda.synchronize()
        cpu = lambda t: None if t is None else t.detach().cpu()   # noqa: E731
        reg = {n: cpu(ar.region(n, self.ws)).clone() for n in self.names}
        P = g["P"]
        o = {"frames": fr, "pr": pr, "pa": pa, "S": cpu(self.S).reshape(P, 64), "h_in": st["h"], "c_in": st["c"],
             "X": reg["X"], "Hs": reg["HS"], "lg": reg["LOGITS"], "ans": reg["ANSWER"], "hid1": reg["HID1"],
             "AO": reg["AO"], "LH": reg["LH"], "logits": cpu(out["logits"]), "values": cpu(out["values"]),
             "gates": None if not opt else cpu(out["gates"]).reshape(B, P, 512),
             "attn": None if not opt else cpu(out["attn"]).reshape(B, P, nq),
             "h_carry": cpu(out["h_out"] if oop else h).reshape(B, P, 128),
             "c": cpu(out["c_out"] if oop else cc).reshape(B, P, 128), "regions": reg}
        if oop:   # the inputs are then only read
            assert torch.equal(cpu(h).reshape(B, P, 128), st["h"]) and torch.equal(cpu(cc).reshape(B, P, 128), st["c"])
        if core:
            o.update(core_h_in=st["core_h"], core_c_in=st["core_c"], q1=reg["Q1"], q2=reg["Q2"], qt=reg["QT"],
                     query_out=None if not opt else cpu(kw["query"]).reshape(B, -1),
                     core_h_out=cpu(kw["core_h_out"] if oop else kw["core_h"]),
                     core_c_out=cpu(kw["core_c_out"] if oop else kw["core_c"]))
            if oop:
                assert torch.equal(cpu(kw["core_h"]), st["core_h"]) and torch.equal(cpu(kw["core_c"]), st["core_c"])
        assert int(ctr.item()) == counter + (1 if opt else 0)
        if opt:
            o.update(actions=cpu(out["actions"]), logp=cpu(out["logp"]), jac=cpu(out["dlogp"]))
            sa, slp = sample_actions(out["logits"], seed=SEED, counter=torch.tensor([counter], dtype=torch.int64, device=dev))
            assert torch.equal(sa, out["actions"]) and torch.equal(slp, out["logp"])
        return o


def _check_draw(o, A, counter):
    """The fused draw against the oracle's restatement on the chain's own logits (draws within fp32 rounding of a
    CDF boundary may differ), its log-probability, and dlogp / dlogits as tests/test_gpu_actor.py holds it."""
    lg = o["logits"]
    ra, rlp, margin = ref_cpu.sample_actions(lg.numpy(), SEED, counter)
    a = o["actions"].numpy()
    sure = margin > 1e-5
    assert np.array_equal(a[sure], ra[sure]), (a, ra, margin)
    assert (a >= 0).all() and (a < A).all()
    ref = torch.log_softmax(lg.double(), -1).gather(1, o["actions"].long()[:, None])[:, 0]
    eps = float(np.finfo(np.float32).eps)
    ref = ref.clamp(np.log(eps), np.log1p(-eps))
    assert float((o["logp"].double() - ref).abs().max()) <= 2e-6 * max(1.0, float(ref.abs().max()))
    ref_jac = torch.nn.functional.one_hot(o["actions"].long(), A).float() - torch.softmax(lg, -1)
    assert float((o["jac"] - ref_jac).abs().max()) <= 1e-6


def _same(a, b, keys):
    for k in keys:
        x, y = (a["regions"][k], b["regions"][k]) if k in a["regions"] else (a[k], b[k])
        assert torch.equal(x, y), k


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_actor_stages_on_their_own_operands(cuda, case):
    H, W, B, nq, A, core, u8, prev, oop = case
    ch = _Chain(cuda, case)
    st0 = R.state0(case)
    o1 = ch.step(st0, 0, 5, oop=False)
    ck = R.check(o1, case, "step 0")
    print("[actor] " + ck.report())
    assert not ck.bad, ck.bad
    _check_draw(o1, A, 5)
    st1 = R.next_state(case, o1)
    assert not torch.equal(st1["h"], st0["h"]) and not torch.equal(st1["c"], st0["c"])
    o2 = ch.step(st1, 1, 6, oop=oop)
    ck = R.check(o2, case, "step 1")
    print("[actor] " + ck.report())
    assert not ck.bad, ck.bad
    _check_draw(o2, A, 6)
    outs = ("logits", "values", "h_carry", "c") + (("core_h_out", "core_c_out") if core else ())
    drawn = ("gates", "attn", "actions", "logp", "jac") + (("query_out",) if core else ())
    # the same step twice out of place from the same inputs: whichever K slice, chunk or LSTMCell workgroup
    # arrives last; and in place: h_out / c_out (core_h_out / core_c_out) change where the state lands, nothing else
    a = o2 if oop else ch.step(st1, 1, 6, oop=True)
    _same(a, ch.step(st1, 1, 6, oop=True), outs + drawn + ch.names)
    _same(a, ch.step(st1, 1, 6, oop=False) if oop else o2, outs + drawn + ch.names)
    # attn, gates, actions (and query) NULL: everything else as before
    _same(o2, ch.step(st1, 1, 6, oop=oop, opt=False), outs + ch.names)


def test_expf_term_measured(cuda):
    """The measurement behind actor_ref.TAU_EXP: the worst relative error of the attention map against the fp64
    softmax of the stored logits, over the workload's grid at B = 16 and the largest grids.  Printed; TAU_EXP is
    4 x the value recorded from this test and the error must stay under it."""
    worst = 0.0
    for cid in ("84x84_B16nq4A256_u8_oop", "210x160_B4nq4A18_f32_noprev", "506x256_B1nq8A18_u8_noprev"):
        case = next(c for c in R.CASES if R.case_id(c) == cid)
        o = _Chain(cuda, case).step(R.state0(case), 0, 0, oop=False)
        A64 = torch.softmax(o["lg"].double(), 1)
        assert float(A64.min()) > 1e-30
        worst = max(worst, float(((o["attn"].double() - A64).abs() / A64).max()))
    print(f"[actor] expf term: worst relative map error {worst:.3e}; TAU_EXP_MEASURED {R.TAU_EXP_MEASURED:.1e}, "
          f"TAU_EXP {R.TAU_EXP:.1e}")
    assert worst <= R.TAU_EXP <= R.TAU_CAP
