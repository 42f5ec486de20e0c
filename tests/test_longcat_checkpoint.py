"""CPU: the host side of running LongCat-Video from a checkpoint folder -- the expected-key table of the loader, the scheduler's
from_config / from_pretrained, the checkpoint audit (headers and JSON only) with its command, and what the entry point
`worldforge_amd.longcat_infer` refuses before any device is touched.  The GPU side is tests/test_gpu_longcat_entry.py."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import longcat_dit as olc
from tests import longcat_ckpt as ck
from tests.fakes import lora_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRUCK = os.path.join(ROOT, "tests", "golden", "truck")


# ---- the loader's table ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [ck.KW, dict(hidden_size=384, depth=3, num_heads=3, caption_channels=96, adaln_tembed_dim=64)])
def test_expected_state_dict_is_the_reference_state_dict(kw):
    from worldforge_amd.longcat_dit import LongCatConfig, expected_state_dict
    want = olc.random_weights(olc.LongCatConfig(**kw), seed=0)
    got = expected_state_dict(LongCatConfig(**kw))
    assert set(got) == set(want), sorted(set(got) ^ set(want))[:8]
    assert all(tuple(want[k].shape) == tuple(got[k]) for k in want)


def test_config_from_dict_fields_ignored_keys_and_class_name():
    from worldforge_amd.longcat_dit import config_from_dict
    c = {**ck.CONFIG_EXTRA, **ck.KW, "patch_size": [1, 2, 2], "text_tokens_zero_pad": True, "enable_bsa": True, "bsa_params": ck.BSA,
         "some_new_field": 3}
    cfg, ctor, unknown = config_from_dict(c)
    assert (cfg.hidden_size, cfg.depth, cfg.num_heads, cfg.caption_channels, cfg.adaln_tembed_dim) == (256, 2, 2, 64, 32)
    assert cfg.patch_size == (1, 2, 2) and cfg.text_tokens_zero_pad is True
    assert ctor == dict(enable_bsa=True, bsa_params=ck.BSA) and unknown == ["some_new_field"]
    with pytest.raises(ValueError, match="WanTransformer3DModel"):
        config_from_dict({**c, "_class_name": "WanTransformer3DModel"})


# ---- the scheduler -----------------------------------------------------------------------------------------------------------------
def test_scheduler_from_config_and_from_pretrained(tmp_path):
    from worldforge_amd.longcat_scheduler import FlowMatchEulerDiscreteScheduler as S
    ck.write_scheduler(str(tmp_path), shift=7.0, num_train_timesteps=500)
    for got in (S.from_config({**ck.SCHEDULER, "shift": 7.0, "num_train_timesteps": 500}), S.from_pretrained(str(tmp_path)),
                S.from_pretrained(str(tmp_path / "scheduler"), subfolder=None)):
        want = S(num_train_timesteps=500, shift=7.0)
        assert torch.equal(got.timesteps, want.timesteps) and torch.equal(got.sigmas, want.sigmas)
        assert got.config.shift == 7.0 and got.config.num_train_timesteps == 500 and got.flow_backend == "farneback"
        got.set_timesteps(4, sigmas=torch.linspace(0.999, 0.0, 4))
        want.set_timesteps(4, sigmas=torch.linspace(0.999, 0.0, 4))
        assert torch.equal(got.timesteps, want.timesteps) and torch.equal(got.sigmas, want.sigmas)
    assert S.from_pretrained(str(tmp_path), flow_backend="tdiff").flow_backend == "tdiff"
    for flag in ("use_dynamic_shifting", "use_karras_sigmas", "stochastic_sampling"):
        with pytest.raises(NotImplementedError):
            S.from_config({**ck.SCHEDULER, flag: True})
    ck.write_scheduler(str(tmp_path), invert_sigmas=True)
    with pytest.raises(NotImplementedError):
        S.from_pretrained(str(tmp_path))


# ---- the audit -----------------------------------------------------------------------------------------------------------------------
def _clean_folder(root, W=None, shards=2):
    W = ck.weights() if W is None else W
    ck.write_dit(root, W, shards=shards)
    ck.write_scheduler(root)
    ck.write_lora(root, "cfg_step_lora", lora_state(olc.LongCatConfig(**ck.KW)))
    return W


def _classes(c):
    return c["missing"], c["unexpected"], [w["key"] for w in c["wrong_shape"]]


def test_audit_of_a_clean_sharded_folder_is_empty_and_exits_0(tmp_path, capsys):
    from worldforge_amd import checkpoint
    W = _clean_folder(str(tmp_path))
    rep = checkpoint.audit(str(tmp_path))
    assert rep["ok"] and set(rep["components"]) == {"dit", "scheduler", "lora/cfg_step_lora"}
    for name, c in rep["components"].items():
        assert _classes(c) == ([], [], []) and c["refused"] == [], name
        assert c["index"]["missing_shards"] == [] and c["index"]["unindexed"] == [] and c["index"]["index_only"] == []
    d = rep["components"]["dit"]
    assert d["dtypes"] == {"F32": len(W)} and d["bytes"] == sum(v.numel() * 4 for v in W.values())
    assert d["index"]["index"] == "diffusion_pytorch_model.safetensors.index.json"
    s = rep["components"]["scheduler"]
    assert s["values"]["shift"] == 3.0 and s["values"]["num_train_timesteps"] == 1000 and s["kind"] == "FlowMatchEulerDiscreteScheduler"
    assert checkpoint.main([str(tmp_path)]) == 0
    assert "OK" in capsys.readouterr().out
    assert checkpoint.main([str(tmp_path), "--json"]) == 0
    assert json.loads(capsys.readouterr().out)["ok"] is True
    with pytest.raises(FileNotFoundError):
        checkpoint.audit(str(tmp_path / "nowhere"))


def test_audit_reports_each_fault_in_its_class_by_name(tmp_path, capsys):
    from worldforge_amd import checkpoint
    W = ck.weights()
    W["blocks.1.attn.q_norm.scale"] = W.pop("blocks.1.attn.q_norm.weight")          # renamed
    W["blocks.0.attn.rope.freqs"] = torch.zeros(8)                                  # extra
    W["blocks.0.ffn.w2.weight"] = W["blocks.0.ffn.w2.weight"].t().contiguous()      # wrong shape
    ck.write_dit(str(tmp_path), W, shards=2)
    ck.write_scheduler(str(tmp_path), use_karras_sigmas=True)
    lora = lora_state(olc.LongCatConfig(**ck.KW))
    H = "___lorahyphen___"
    orphan = "lora" + H + "blocks" + H + "7" + H + "attn" + H + "proj"
    lora[orphan + ".lora_down.weight"], lora[orphan + ".lora_up.weight"] = torch.zeros(8, 256), torch.zeros(256, 8)
    conv = "lora" + H + "x_embedder" + H + "proj"                                   # a Conv3d, not a Linear
    lora[conv + ".lora_down.weight"], lora[conv + ".lora_up.weight"] = torch.zeros(8, 64), torch.zeros(256, 8)
    bad = "lora" + H + "blocks" + H + "0" + H + "attn" + H + "proj"
    lora[bad + ".lora_up.weight"] = torch.zeros(128, 8)                             # up-projection of the wrong height
    ck.write_lora(str(tmp_path), "refinement_lora", lora)
    rep = checkpoint.audit(str(tmp_path))
    assert not rep["ok"]
    d = rep["components"]["dit"]
    assert _classes(d) == (["blocks.1.attn.q_norm.weight"], ["blocks.0.attn.rope.freqs", "blocks.1.attn.q_norm.scale"], ["blocks.0.ffn.w2.weight"])
    assert d["wrong_shape"][0]["found"] == [768, 256] and d["wrong_shape"][0]["expected"] == [256, 768]
    assert rep["components"]["scheduler"]["refused"] == ["use_karras_sigmas=True"]
    lo = rep["components"]["lora/refinement_lora"]
    assert lo["unexpected"] == [orphan + ".lora_down.weight", conv + ".lora_down.weight"] and lo["missing"] == []
    assert [w["key"] for w in lo["wrong_shape"]] == [bad + ".lora_down.weight"]
    assert checkpoint.main([str(tmp_path)]) == 1
    out = capsys.readouterr().out
    for name in ("blocks.1.attn.q_norm.weight", "blocks.0.attn.rope.freqs", "blocks.0.ffn.w2.weight", orphan, "use_karras_sigmas"):
        assert name in out, name


def test_audit_names_a_shard_that_is_missing_from_disk_and_tensors_outside_the_index(tmp_path):
    from safetensors.torch import save_file
    from worldforge_amd import checkpoint
    W = _clean_folder(str(tmp_path))
    folder = tmp_path / "dit"
    gone = "diffusion_pytorch_model-00002-of-00002.safetensors"
    kept = "diffusion_pytorch_model-00001-of-00002.safetensors"
    os.remove(folder / gone)
    first = {k: v for k, v in checkpoint.load_file(str(folder / kept)).items()}
    save_file({**{k: v.clone() for k, v in first.items()}, "stray.weight": torch.zeros(3)}, str(folder / kept))
    rep = checkpoint.audit(str(tmp_path))
    d = rep["components"]["dit"]
    assert not rep["ok"] and d["index"]["missing_shards"] == [gone] and d["index"]["unindexed"] == ["stray.weight"]
    assert d["missing"] == sorted(W)[1::2] and d["unexpected"] == [] and d["wrong_shape"] == []
    assert checkpoint.main([str(tmp_path)]) == 1


def test_unindexed_tensors_are_reported_only_and_the_text_report_lists_ten_names_per_class(tmp_path, capsys):
    from safetensors.torch import save_file
    from worldforge_amd import checkpoint
    _clean_folder(str(tmp_path))
    kept = str(tmp_path / "dit" / "diffusion_pytorch_model-00001-of-00002.safetensors")
    first = {k: v.clone() for k, v in checkpoint.load_file(kept).items()}
    save_file({**first, "stray.weight": torch.zeros(3)}, kept)
    rep = checkpoint.audit(str(tmp_path))
    assert rep["components"]["dit"]["index"]["unindexed"] == ["stray.weight"] and rep["components"]["dit"]["unexpected"] == []
    assert rep["ok"] and checkpoint.main([str(tmp_path)]) == 0          # load_dir never reads it
    assert "stray.weight" in capsys.readouterr().out
    W = ck.weights()
    extra = [f"extra.{i:02d}.weight" for i in range(12)]
    W.update({k: torch.zeros(2) for k in extra})
    ck.write_dit(str(tmp_path), W, shards=1)
    os.remove(tmp_path / "dit" / "diffusion_pytorch_model.safetensors.index.json")
    for fn in os.listdir(tmp_path / "dit"):
        if "-of-" in fn:
            os.remove(tmp_path / "dit" / fn)
    assert checkpoint.audit(str(tmp_path))["components"]["dit"]["unexpected"] == extra
    assert checkpoint.main([str(tmp_path)]) == 1
    out = capsys.readouterr().out
    assert "unexpected: 12" in out and "and 2 more" in out
    assert all(k in out for k in extra[:10]) and not any(k in out for k in extra[10:])


@pytest.mark.parametrize("which", ["scheduler/scheduler_config.json", "dit/config.json"])
def test_a_json_file_that_does_not_parse_is_a_refused_component_not_a_traceback(tmp_path, capsys, which):
    from worldforge_amd import checkpoint
    _clean_folder(str(tmp_path))
    (tmp_path / which).write_text("{bad")
    rep = checkpoint.audit(str(tmp_path))
    c = rep["components"][which.split("/")[0]]
    assert not rep["ok"] and len(c["refused"]) == 1 and os.path.basename(which) in c["refused"][0] and c["missing"] == []
    assert checkpoint.main([str(tmp_path)]) == 1
    assert "unreadable" in capsys.readouterr().out


def test_audit_of_a_wan_layout_transformer_reports_a_renamed_and_an_extra_key(tmp_path):
    from worldforge_amd import checkpoint
    from worldforge_amd.dit import config_from_diffusers, diffusers_key_map, expected_diffusers_state_dict
    conf = {"_class_name": "WanTransformer3DModel", "num_attention_heads": 2, "attention_head_dim": 128, "ffn_dim": 512, "num_layers": 2,
            "text_dim": 64, "image_dim": 64, "in_channels": 36, "out_channels": 16, "freq_dim": 256, "patch_size": [1, 2, 2]}
    exp = expected_diffusers_state_dict(config_from_diffusers(conf))
    km = diffusers_key_map(2)
    assert {k.rpartition(".")[0] for k in exp if not k.endswith("scale_shift_table")} == set(km)
    W = {k: torch.zeros(s, dtype=torch.bfloat16) for k, s in exp.items()}
    ck.write_weights(str(tmp_path / "transformer"), W)
    (tmp_path / "transformer" / "config.json").write_text(json.dumps(conf))
    assert checkpoint.audit(str(tmp_path))["ok"]
    W["blocks.1.attn2.to_out.weight"] = W.pop("blocks.1.attn2.to_out.0.weight")
    W["blocks.0.attn1.rope_freqs"] = torch.zeros(4)
    W["blocks.0.ffn.net.2.weight"] = torch.zeros(512, 256, dtype=torch.bfloat16)
    ck.write_weights(str(tmp_path / "transformer"), W)
    rep = checkpoint.audit(str(tmp_path))
    c = rep["components"]["transformer"]
    assert not rep["ok"] and c["kind"] == "WanTransformer3DModel"
    assert _classes(c) == (["blocks.1.attn2.to_out.0.weight"], ["blocks.0.attn1.rope_freqs", "blocks.1.attn2.to_out.weight"],
                           ["blocks.0.ffn.net.2.weight"])
    assert c["dtypes"] == {"BF16": len(W) - 1, "F32": 1}
    # a LongCat loader pointed at this folder is refused by the class name
    (tmp_path / "dit").mkdir()
    (tmp_path / "dit" / "config.json").write_text(json.dumps(conf))
    assert any("WanTransformer3DModel" in r for r in checkpoint.audit(str(tmp_path))["components"]["dit"]["refused"])


def test_audit_of_a_vae_folder_is_key_coverage_by_the_key_map(tmp_path):
    from worldforge_amd import checkpoint
    from worldforge_amd.vae import diffusers_key_map
    bases = sorted(diffusers_key_map())
    W = {b + ".weight": torch.zeros(1) for b in bases}
    W["encoder.nope.weight"] = torch.zeros(1)
    del W[bases[5] + ".weight"]
    ck.write_weights(str(tmp_path / "vae"), W)
    c = checkpoint.audit(str(tmp_path))["components"]["vae"]
    assert c["missing"] == [bases[5] + ".*"] and c["unexpected"] == ["encoder.nope.weight"] and c["wrong_shape"] == []


def test_audit_reads_headers_only(tmp_path):
    """Every weight file cut off right behind its header: the audit still succeeds, the loader's reader does not."""
    from worldforge_amd import checkpoint
    _clean_folder(str(tmp_path))
    cut = 0
    for sub in ("dit", "lora"):
        for fn in os.listdir(tmp_path / sub):
            if fn.endswith(".safetensors"):
                p = str(tmp_path / sub / fn)
                _, base = checkpoint.read_header(p)
                os.truncate(p, base + 16)
                cut += 1
    assert cut == 3
    rep = checkpoint.audit(str(tmp_path))
    assert rep["ok"] and rep["components"]["dit"]["bytes"] > 0
    with pytest.raises(ValueError):
        checkpoint.load_dir(str(tmp_path / "dit"))


# ---- the entry point, before any device -------------------------------------------------------------------------------------------
def test_cli_has_the_reference_arguments_and_defaults():
    """run_longcat_worldforge_single.py:503-556: same flags, same defaults; and this engine's additions."""
    from worldforge_amd import longcat_infer
    a = vars(longcat_infer.build_parser().parse_args(["--checkpoint_dir", "/nowhere", "--video-ref", TRUCK]))
    want = dict(checkpoint_dir="/nowhere", context_parallel_size=1, enable_compile=False, use_distill=False, video_ref=TRUCK, image=None,
                prompt=None, scene=None, negative_prompt=None, resolution="480p", num_frames=93, num_inference_steps=50, guidance_scale=4.0,
                seed=42, fps=15, guided=False, resample_steps=3, guide_steps=20, resample_round=20, omega=1.8, omega_resample=1.0,
                soften_mask=False, transition_distance=15, decay_type="sine", use_pca_channel_selection=False, static="False",
                max_replace=None, output="output_i2v.mp4", save_png=False, enable_upscale=False, t_thresh=0.6,
                embeds=None, height=None, width=None, upscale_height=704, upscale_width=1280, device="cuda:0", dit_precision="bf16",
                vae_precision="bf16", extend_windows=0, num_cond_frames=13, no_kv_cache=False, refine_kv_cache=False)
    assert a == want, {k: (a.get(k), want.get(k)) for k in set(a) | set(want) if a.get(k) != want.get(k)}


def test_the_entry_refuses_before_any_device_is_touched(tmp_path, monkeypatch):
    from worldforge_amd import longcat_infer
    from worldforge_amd.longcat_pipeline import LongCatVideoPipeline

    def no_loading(*a, **k):
        raise AssertionError("the models were loaded before the arguments were checked")

    monkeypatch.setattr(LongCatVideoPipeline, "from_pretrained", classmethod(no_loading))
    emb = str(tmp_path / "e.npz")
    np.savez(emb, prompt_embeds=np.zeros((1, 1, 4, 64), np.float32), prompt_attention_mask=np.ones((1, 4), np.int64),
             negative_prompt_embeds=np.zeros((1, 1, 4, 64), np.float32), negative_prompt_attention_mask=np.ones((1, 4), np.int64))
    with pytest.raises(ValueError, match="does not exist"):
        longcat_infer.main(["--checkpoint_dir", str(tmp_path / "nowhere"), "--video-ref", TRUCK, "--num-frames", "9", "--embeds", emb])
    with pytest.raises(ValueError, match="context_parallel_size"):
        longcat_infer.main(["--checkpoint_dir", str(tmp_path), "--video-ref", TRUCK, "--num-frames", "9", "--embeds", emb,
                            "--context_parallel_size", "2"])
    for n in (13, 5):    # the truck sequence holds 9 warped frames: neither padded nor truncated
        with pytest.raises(ValueError, match="frames"):
            longcat_infer.main(["--checkpoint_dir", str(tmp_path), "--video-ref", TRUCK, "--num-frames", str(n), "--embeds", emb])
    with pytest.raises(ValueError, match="cfg_step_lora"):       # --use_distill without its LoRA file
        longcat_infer.main(["--checkpoint_dir", str(tmp_path), "--video-ref", TRUCK, "--num-frames", "9", "--embeds", emb, "--use_distill"])
    with pytest.raises(ValueError, match="embeds"):              # neither --embeds nor a text encoder in the folder
        longcat_infer.main(["--checkpoint_dir", str(tmp_path), "--video-ref", TRUCK, "--num-frames", "9"])
    with pytest.raises(AssertionError, match="loaded"):          # and with nothing to refuse, loading is the next thing that happens
        longcat_infer.main(["--checkpoint_dir", str(tmp_path), "--video-ref", TRUCK, "--num-frames", "9", "--embeds", emb])


def test_pick_size_and_what_run_picks_for_a_16_to_9_input(tmp_path, monkeypatch):
    """Without --height / --width the area rule decides: a 16:9 image gives 464 x 832 at 480p -- NOT the 480 x 832 of the reference's
    bucket table (the stated deviation) -- and 720 x 1280 at 720p; --height / --width are taken as they are."""
    from PIL import Image
    from worldforge_amd import harness, longcat_infer
    from worldforge_amd.longcat_pipeline import LongCatVideoPipeline
    for hw in ((1080, 1920), (720, 1280), (576, 1024), (360, 640)):
        assert longcat_infer.pick_size(*hw, "480p") == (464, 832) and longcat_infer.pick_size(*hw, "720p") == (720, 1280)
    assert longcat_infer.pick_size(480, 832, "480p") == (480, 832)
    assert longcat_infer.pick_size(1080, 1920, "480p", 480, 832) == (480, 832)
    with pytest.raises(ValueError, match="together"):
        longcat_infer.pick_size(1080, 1920, "480p", 480, None)
    ref = tmp_path / "ref"
    ref.mkdir()
    for i in range(5):
        Image.new("RGB", (320, 180), (i * 20, 0, 0)).save(ref / f"warp_{i:02d}.png")
        Image.new("L", (320, 180), 255).save(ref / f"mask_{i:02d}.png")
    Image.new("RGB", (300, 300)).save(tmp_path / "square.png")
    emb = str(tmp_path / "e.npz")
    np.savez(emb, prompt_embeds=np.zeros((1, 1, 4, 64), np.float32), prompt_attention_mask=np.ones((1, 4), np.int64))
    picked = []

    class Reached(Exception):
        pass

    def record(*a, size=None, **k):
        picked.append(size)
        raise Reached

    stub = type("Pipe", (), {"dit": None})()
    monkeypatch.setattr(LongCatVideoPipeline, "from_pretrained", classmethod(lambda cls, *a, **k: stub))
    monkeypatch.setattr(harness, "prepare_inputs", record)
    argv = ["--checkpoint_dir", str(tmp_path), "--video-ref", str(ref), "--num-frames", "5", "--embeds", emb, "--guidance-scale", "1.0",
            "--device", "cpu"]
    for more in ([], ["--resolution", "720p"], ["--height", "480", "--width", "832"], ["--image", str(tmp_path / "square.png")]):
        with pytest.raises(Reached):
            longcat_infer.main(argv + more)
    assert picked == [(464, 832), (720, 1280), (480, 832), (624, 624)]


def test_embeds_file_round_trip_and_missing_keys(tmp_path):
    from worldforge_amd import longcat_infer
    g = torch.Generator().manual_seed(1)
    pe, ne = torch.randn(1, 1, 24, 64, generator=g), torch.randn(1, 1, 24, 64, generator=g)
    pm, nm = torch.zeros(1, 24, dtype=torch.int64), torch.zeros(1, 24, dtype=torch.int64)
    pm[:, :19], nm[:, :7] = 1, 1
    p = str(tmp_path / "e.npz")
    np.savez(p, prompt_embeds=pe.numpy(), prompt_attention_mask=pm.numpy(), negative_prompt_embeds=ne.numpy(), negative_prompt_attention_mask=nm.numpy())
    e = longcat_infer.load_embeds(p, "cpu", negative=True)
    assert torch.equal(e["prompt_embeds"], pe.to(torch.bfloat16)) and torch.equal(e["negative_prompt_attention_mask"], nm)
    assert set(longcat_infer.load_embeds(p, "cpu", negative=False)) == {"prompt_embeds", "prompt_attention_mask"}
    from safetensors.torch import save_file
    q = str(tmp_path / "e.safetensors")
    save_file({"prompt_embeds": pe.to(torch.bfloat16), "prompt_attention_mask": pm}, q)
    e2 = longcat_infer.load_embeds(q, "cpu", negative=False)
    assert torch.equal(e2["prompt_embeds"], pe.to(torch.bfloat16)) and torch.equal(e2["prompt_attention_mask"], pm)
    with pytest.raises(ValueError, match="missing"):
        longcat_infer.load_embeds(q, "cpu", negative=True)
    np.savez(p, prompt_embeds=pe[0].numpy(), prompt_attention_mask=pm.numpy())
    with pytest.raises(ValueError, match="expected"):
        longcat_infer.load_embeds(p, "cpu", negative=False)
