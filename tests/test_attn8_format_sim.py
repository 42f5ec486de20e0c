"""tools/attn8_format_sim.py, the CPU simulation behind the go / no-go decision on an 8-bit self-attention mode:
its own sanity, each rounding against what its number format allows, and the gate itself on a reduced case.  No GPU."""
import importlib.util
import os

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("attn8_format_sim", os.path.join(ROOT, "tools", "attn8_format_sim.py"))
sim = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(sim)


def _case(gain, seed, Lq=64, Lk=1000):
    q, k, v = (t[0] for t in sim.make_qkv(Lq, Lk, gain, seed))
    return q, k, v, Lk, sim.exact_attention(q, k, v, Lk)


def test_without_roundings_is_exact_attention():
    q, k, v, Lk, ref = _case(3, 1)
    got, same = sim.sim_attention(q, k, v, Lk, round_qk=False, round_p=False, round_v=False)
    assert sim.rel(got, ref) <= 1e-12 and sim.rel(same, ref) <= 1e-12


def test_row_quantizer_restatement():
    x = torch.zeros(1, 3, 128)
    x[0, 0, :3] = torch.tensor([127.0, -63.5, 0.4])
    x[0, 1, 7] = float("nan")
    q8, s = sim.ref_quant_rows(x.to(torch.bfloat16), 3)
    assert s[0, 0] == 1.0 and q8[0, 0, :3].tolist() == [127, -64, 0]      # -63.5 rounds to even
    assert torch.isnan(s[0, 1]) and not q8[0, 1].any()                     # a NaN row: scale NaN, elements 0
    assert s[0, 2] == 0 and not q8[0, 2].any()                             # an all-zero row
    q8, s = sim.ref_quant_rows(x.to(torch.bfloat16), 0)
    assert not q8.any() and not s.any()                                    # padded rows


def test_each_rounding_within_its_format():
    """Relative steps: INT8 rows 2^-7 of the row maximum, e4m3 2^-3 of the element (half of it at most per rounding).  A softmax-weighted
    sum of independently rounded terms cannot exceed the per-element bound of its format: 2^-4 for e4m3 elements (V, P); the score error
    |q||k| 2^-7 enters through exp2, below that bound at these gains."""
    q, k, v, Lk, ref = _case(3, 2)
    e_qk = sim.rel(sim.sim_attention(q, k, v, Lk, round_p=False, round_v=False)[0], ref)
    e_p = sim.rel(sim.sim_attention(q, k, v, Lk, round_qk=False, round_v=False)[0], ref)
    e_v = sim.rel(sim.sim_attention(q, k, v, Lk, round_qk=False, round_p=False)[0], ref)
    assert 0 < e_qk < 2.0 ** -4 and 0 < e_p < 2.0 ** -4 and 0 < e_v < 2.0 ** -4


def test_gate_reads_no_go():
    """The gate of DESIGN.md section 4e on the 256 x 4096 case at q gain 3: the whole format must stay within a quarter of the MX-e4m3
    Q / K / V error.  It does not (3.7e-2 against 2.3e-2), and the MX-e4m3 V^T alone (2.7e-2) is already past it: what is recorded as the
    reason the mode was not built into the DiTs.  If a change to the format makes this test fail, section 4e is out of date."""
    (_, _, gain, e_all, e_qk, e_p, e_v), = sim.table(shapes=((256, 4096),), gains=(3,))
    print(f"[attn8 format, 256 x 4096, gain {gain}] e_fmt {e_all:.3e}: INT8 QK {e_qk:.3e}, e4m3 P {e_p:.3e}, MX-e4m3 V {e_v:.3e}; "
          f"gate {sim.MX_QKV_GAIN3 / 4:.3e}")
    assert e_all > sim.MX_QKV_GAIN3 / 4 and e_v > sim.MX_QKV_GAIN3 / 4
    assert e_qk < sim.MX_QKV_GAIN3 / 4   # the INT8 scores alone would have passed: the premise about Q K^T holds, the V^T format decides
