"""CPU: the host side of the switchable LoRA adapters -- argument validation of wf_lora_fold (every rejected call returns WF_EINVAL with
wf_last_error() set before any device work) and the bookkeeping of load_lora / enable_loras / disable_all_loras on a "cpu"-device LongCat
DiT (parsing, strictness, scales, the state machine with the device call replaced)."""
import pytest
import torch

from oracle import longcat_dit as olc
from worldforge_amd import _ffi

EINVAL = -1
A16 = 1 << 20  # a 16-byte aligned fake address: never dereferenced, every call below is rejected first
H = "___lorahyphen___"
KW = dict(hidden_size=256, depth=2, num_heads=2, caption_channels=64, adaln_tembed_dim=64)


def _fold(**kw):
    a = dict(base=A16, out=A16, N=96, K=64, n=1)
    for j in range(4):
        a.update({f"U{j}": A16, f"D{j}": A16, f"rank{j}": 8, f"nsep{j}": 1, f"scale{j}": 1.0})
    a.update(kw)
    flat = [x for j in range(4) for x in (a[f"U{j}"], a[f"D{j}"], a[f"rank{j}"], a[f"nsep{j}"], a[f"scale{j}"])]
    return _ffi.lib().wf_lora_fold(a["base"], a["out"], a["N"], a["K"], a["n"], *flat, None)


@pytest.mark.parametrize("bad", [
    dict(base=None), dict(out=None), dict(U0=None), dict(D0=None), dict(n=2, U1=None), dict(n=4, D3=None),   # null pointers
    dict(N=0), dict(N=-3),
    dict(K=60), dict(K=4), dict(K=0),                                                        # K % 8 != 0
    dict(base=A16 + 8), dict(out=A16 + 2), dict(U0=A16 + 4), dict(D0=A16 + 8), dict(n=2, U1=A16 + 2),  # misaligned pointers
    dict(n=0), dict(n=5), dict(n=-1),                                                        # n_adapters outside 1..4
    dict(nsep0=5), dict(nsep0=0), dict(N=100, nsep0=3), dict(n=2, nsep1=7),                  # N % nsep != 0
    dict(rank0=0), dict(rank0=4), dict(rank0=12), dict(rank0=264), dict(n=3, rank2=20),      # a rank the kernel does not take
    dict(n=4, rank0=256, rank1=256, rank2=256, rank3=256),                                   # ... or more operand panel than the LDS holds
])
def test_lora_fold_rejects(bad):
    assert _fold(**bad) == EINVAL
    assert _ffi.lib().wf_last_error()


def _model(W=None):
    from worldforge_amd.longcat_dit import LongCatConfig, LongCatVideoTransformer3DModel
    W = olc.random_weights(olc.LongCatConfig(**KW), seed=21) if W is None else W
    return LongCatVideoTransformer3DModel(LongCatConfig(**KW), "cpu").load_state_dict(W)


def _name(module):
    return "lora" + H + module.replace(".", H)


def _entry(module, o, k, rank=8, nsep=1, seed=0):
    g = torch.Generator().manual_seed(seed)
    n = _name(module)
    sd = {n + ".lora_down.weight": torch.randn(nsep * rank, k, generator=g)}
    if nsep == 1:
        sd[n + ".lora_up.weight"] = torch.randn(o, rank, generator=g)
    else:
        for b in range(nsep):
            sd[n + f".lora_up.blocks.{b}.weight"] = torch.randn(o // nsep, rank, generator=g)
    return sd


def test_load_lora_is_strict_and_leaves_lora_dict_unchanged():
    m = _model()
    good = _entry("blocks.0.attn.proj", 256, 256)
    m.load_lora(good, "good")
    before = dict(m.lora_dict)
    for module in ("blocks.9.attn.proj", "blocks.0.attn.nothing", "blocks.2.adaLN_modulation.1", "x_embedder.proj", "blocks.0.attn.q_norm"):
        with pytest.raises(KeyError):
            m.load_lora({**good, **_entry(module, 256, 256)}, "bad")
    with pytest.raises(KeyError):   # a down-projection without any up-projection
        m.load_lora({_name("blocks.0.attn.proj") + ".lora_down.weight": torch.zeros(8, 256)}, "bad")
    qkv17 = _entry("blocks.0.attn.qkv", 768, 256, nsep=2)
    qkv17[_name("blocks.0.attn.qkv") + ".lora_down.weight"] = torch.zeros(17, 256)
    for sd in (_entry("blocks.0.attn.proj", 256, 128),             # K of the down-projection
               _entry("blocks.0.attn.proj", 512, 256),             # rows of the up-projection
               qkv17,                                              # 17 ranks do not split over 2 up-blocks
               _entry("blocks.0.ffn.w1", 2 * 768, 256),            # w1 is one half of w13, not all of it
               _entry("blocks.0.cross_attn.kv_linear", 256, 256, nsep=2)):
        with pytest.raises(ValueError):
            m.load_lora({**good, **sd}, "bad")
        with pytest.raises(ValueError):
            m.load_lora({**good, **sd}, "good")   # nor is an existing key replaced by a rejected adapter
    assert list(m.lora_dict) == ["good"] and m.lora_dict["good"] is before["good"] and m.active_loras == []


def test_scales_targets_and_bf16_factors():
    m = _model()
    Hd = m.cfg.ffn_hidden
    sd = {}
    sd.update(_entry("blocks.1.attn.qkv", 768, 256, nsep=3, seed=1))
    sd.update(_entry("blocks.0.ffn.w3", Hd, 256, seed=2))
    sd.update(_entry("blocks.1.adaLN_modulation.1", 6 * 256, 64, seed=3))
    sd.update(_entry("blocks.0.ffn.w2", 256, Hd, rank=4, seed=4))
    sd[_name("blocks.1.attn.qkv") + ".alpha_scale"] = torch.tensor(0.25)
    m.load_lora(sd, "k", multiplier=0.8, lora_network_dim=8, lora_network_alpha=4)
    parts = {(p.wkey, p.row0): p for p in m.lora_dict["k"]}
    assert sorted(parts) == [("ada.w", 6 * 256), ("blocks.0.ffn.w13", Hd), ("blocks.0.ffn.w2", 0), ("blocks.1.attn.qkv.w", 0)]
    q = parts[("blocks.1.attn.qkv.w", 0)]
    assert q.scale == pytest.approx(0.8 * 0.25) and q.nsep == 3 and q.U.shape == (768, 8) and q.D.shape == (24, 256)   # .alpha_scale wins
    n = _name("blocks.1.attn.qkv")
    assert torch.equal(q.U, torch.cat([sd[n + f".lora_up.blocks.{b}.weight"] for b in range(3)], 0).to(torch.bfloat16))
    assert torch.equal(q.D, sd[n + ".lora_down.weight"].to(torch.bfloat16)) and q.U.dtype == q.D.dtype == torch.bfloat16
    assert parts[("blocks.0.ffn.w13", Hd)].scale == pytest.approx(0.8 * 4 / 8)    # no .alpha_scale: alpha / dim
    assert parts[("ada.w", 6 * 256)].U.shape == (6 * 256, 8)
    w2 = parts[("blocks.0.ffn.w2", 0)]   # rank 4 is zero-padded to the kernel's 8-rank operand slot
    assert w2.U.shape == (256, 8) and w2.D.shape == (8, Hd) and not w2.U[:, 4:].any() and not w2.D[4:].any()
    m.load_lora(sd, "dflt")   # the defaults: dim 128, alpha 64
    assert {p.wkey: p.scale for p in m.lora_dict["dflt"]}["blocks.0.ffn.w2"] == pytest.approx(0.5)


def test_bookkeeping_across_enable_and_disable(monkeypatch):
    from worldforge_amd import ops
    calls = []

    def fake_fold(base, out, adapters):
        calls.append((tuple(base.shape), len(adapters)))
        out.copy_(base)
        return out

    monkeypatch.setattr(ops, "lora_fold", fake_fold)
    m = _model()
    base = m.w
    a = {**_entry("blocks.0.attn.proj", 256, 256, seed=1), **_entry("blocks.0.ffn.w1", m.cfg.ffn_hidden, 256, seed=2)}
    b = _entry("blocks.0.attn.proj", 256, 256, seed=3)
    m.load_lora(a, "A")
    m.load_lora(b, "B")
    assert isinstance(m.lora_dict, dict) and isinstance(m.active_loras, list) and m.active_loras == [] and not calls and m.w is base
    m.enable_loras(["A", "nope", "A"])
    assert m.active_loras == ["A"] and sorted(calls) == [((256, 256), 1), ((m.cfg.ffn_hidden, 256), 1)]
    assert m.w is not base and m.base_w is base and m.w["blocks.0.attn.proj.w"] is not base["blocks.0.attn.proj.w"]
    assert m.w["blocks.1.attn.proj.w"] is base["blocks.1.attn.proj.w"] and m._wl is m.w
    assert torch.equal(m.w["blocks.0.ffn.w13"], base["blocks.0.ffn.w13"])   # (the stand-in copies; the w3 half is copied by the model)
    buf = m.w["blocks.0.attn.proj.w"]
    del calls[:]
    m.enable_loras(["B", "A"])   # both adapters of attn.proj go into ONE launch
    assert m.active_loras == ["B", "A"] and sorted(calls) == [((256, 256), 2), ((m.cfg.ffn_hidden, 256), 1)]
    assert m.w["blocks.0.attn.proj.w"] is buf
    del calls[:]
    m.load_lora(b, "A")          # replacing an ACTIVE adapter folds again; an inactive one does not
    assert sorted(calls) == [((256, 256), 2)] and "blocks.0.ffn.w13" not in {k for k in m.w if m.w[k] is not base[k]}
    m.disable_all_loras()
    del calls[:]
    m.load_lora(a, "A")
    assert m.active_loras == [] and m.w is base and not calls and sorted(m.lora_dict) == ["A", "B"]
    m.enable_loras(["B"])
    m.w = dict(base)             # a new base deactivates, the loaded adapters stay
    assert m.active_loras == [] and sorted(m.lora_dict) == ["A", "B"] and m.w is m.base_w


def test_no_device_no_fold():
    m = _model()
    m.load_lora(_entry("blocks.0.attn.proj", 256, 256), "A")
    with pytest.raises(RuntimeError):   # there is no CPU fallback for the switch
        m.enable_loras(["A"])


def test_load_lora_reads_a_safetensors_file(tmp_path):
    import json
    import struct
    sd = {**_entry("blocks.0.attn.proj", 256, 256, seed=5), _name("blocks.0.attn.proj") + ".alpha_scale": torch.tensor(0.75)}
    hdr, blob = {}, b""
    for k, v in sd.items():
        raw = v.contiguous().numpy().tobytes()
        hdr[k] = {"dtype": "F32", "shape": list(v.shape), "data_offsets": [len(blob), len(blob) + len(raw)]}
        blob += raw
    head = json.dumps(hdr).encode()
    path = tmp_path / "adapter.safetensors"
    path.write_bytes(struct.pack("<Q", len(head)) + head + blob)
    m, ref = _model(), _model()
    m.load_lora(str(path), "file", multiplier=2.0)
    ref.load_lora(sd, "dict", multiplier=2.0)
    (p,), (q,) = m.lora_dict["file"], ref.lora_dict["dict"]
    assert p.wkey == q.wkey == "blocks.0.attn.proj.w" and p.scale == q.scale == pytest.approx(1.5)
    assert torch.equal(p.U, q.U) and torch.equal(p.D, q.D)
