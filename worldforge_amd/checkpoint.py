"""Checkpoint reader for the diffusers directories the reference loads (INFER:179-197: `AutoencoderKLWan.from_pretrained(...,
subfolder="vae")`, `WanImageToVideoPipeline.from_pretrained(model_id, ...)` -> `transformer/`): safetensors files, single or sharded
with a `*.safetensors.index.json` weight map.

The safetensors container is parsed here directly (8-byte little-endian header length, a JSON header {name: {dtype, shape,
data_offsets}}, then the raw little-endian tensor bytes) and memory-mapped, so a 28 GB transformer checkpoint is never copied on the
host more than once per tensor on its way to HBM.  No dependency on the `safetensors` package (tests use it as the writer).

`audit(path)` / `python -m worldforge_amd.checkpoint PATH [--json]` say what a checkpoint folder lacks BEFORE anything is loaded: per
component (`dit/` LongCat, `transformer/` Wan, `vae/`, `text_encoder/`, `image_encoder/`, `scheduler/`, `lora/*.safetensors`) the keys the loader needs and the folder
lacks, the keys no loader consumes, wrong shapes, dtypes, bytes and the consistency of a shard index.  It reads safetensors HEADERS and
JSON files only, never tensor data, and touches no GPU."""
from __future__ import annotations

import glob
import json
import mmap
import os
import struct
import sys
from typing import Dict, Iterable, List, Optional, Tuple

import numpy as np
import torch

_DTYPES = {
    "F64": (torch.float64, 8), "F32": (torch.float32, 4), "F16": (torch.float16, 2), "BF16": (torch.bfloat16, 2),
    "I64": (torch.int64, 8), "I32": (torch.int32, 4), "I16": (torch.int16, 2), "I8": (torch.int8, 1), "U8": (torch.uint8, 1),
    "BOOL": (torch.bool, 1),
}


def read_header(path: str):
    """-> (header dict without __metadata__, byte offset of the data section)."""
    with open(path, "rb") as f:
        raw = f.read(8)
        if len(raw) != 8:
            raise ValueError(f"{path}: not a safetensors file (shorter than its 8-byte header length)")
        (n,) = struct.unpack("<Q", raw)
        size = os.path.getsize(path)
        if n <= 0 or 8 + n > size:
            raise ValueError(f"{path}: not a safetensors file (header length {n} exceeds the file size {size})")
        hdr = json.loads(f.read(n).decode("utf-8"))
    hdr.pop("__metadata__", None)
    return hdr, 8 + n


def load_file(path: str, names: Optional[Iterable[str]] = None) -> Dict[str, torch.Tensor]:
    """All (or the named) tensors of one safetensors file as CPU tensors backed by a private copy-on-write memory map."""
    hdr, base = read_header(path)
    want = set(hdr) if names is None else set(names)
    missing = want - set(hdr)
    if missing:
        raise KeyError(f"{path}: tensors not in the file: {sorted(missing)[:5]}")
    size = os.path.getsize(path)
    out: Dict[str, torch.Tensor] = {}
    with open(path, "rb") as f:
        mm = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_COPY)
    buf = np.frombuffer(mm, dtype=np.uint8)
    for name in sorted(want):
        e = hdr[name]
        if e["dtype"] not in _DTYPES:
            raise ValueError(f"{path}: tensor {name!r} has unsupported dtype {e['dtype']}")
        dt, isz = _DTYPES[e["dtype"]]
        lo, hi = e["data_offsets"]
        numel = int(np.prod(e["shape"])) if e["shape"] else 1
        if hi - lo != numel * isz or base + hi > size or lo < 0:
            raise ValueError(f"{path}: tensor {name!r} has inconsistent offsets {lo}:{hi} for shape {e['shape']} {e['dtype']}")
        t = torch.from_numpy(buf[base + lo:base + hi])
        out[name] = (t.view(dt) if numel else torch.empty(0, dtype=dt)).reshape(e["shape"])
    return out


def load_dir(folder: str) -> Dict[str, torch.Tensor]:
    """A diffusers component directory: `<name>.safetensors.index.json` + shards, or the single `*.safetensors` file."""
    if os.path.isfile(folder):
        return load_file(folder)
    files = sorted(os.listdir(folder))
    idx = [f for f in files if f.endswith(".safetensors.index.json")]
    if idx:
        if len(idx) > 1:
            raise ValueError(f"{folder}: several index files {idx}")
        with open(os.path.join(folder, idx[0])) as f:
            wm = json.load(f)["weight_map"]
        by_file: Dict[str, list] = {}
        for name, fn in wm.items():
            by_file.setdefault(fn, []).append(name)
        out: Dict[str, torch.Tensor] = {}
        for fn, names in sorted(by_file.items()):
            p = os.path.join(folder, fn)
            if not os.path.exists(p):
                raise FileNotFoundError(f"{folder}: shard {fn} named by {idx[0]} is missing")
            out.update(load_file(p, names))
        return out
    st = [f for f in files if f.endswith(".safetensors")]
    if len(st) != 1:
        raise FileNotFoundError(f"{folder}: expected one *.safetensors file or an index, found {st}")
    return load_file(os.path.join(folder, st[0]))


# ---- headers only -------------------------------------------------------------------------------------------------------------------
def dir_header(folder: str) -> Tuple[Dict[str, dict], dict]:
    """The tensors a component directory (or a single file) declares, from the safetensors headers alone:
    -> ({name: {"dtype", "shape", "bytes", "file"}}, {"index", "missing_shards", "unindexed", "index_only"}).  With an index, a shard it
    names that is absent is listed (not raised), as are tensors a shard holds that the index does not list (load_dir never reads them)
    and tensors the index lists that their shard does not hold."""
    info = {"index": None, "missing_shards": [], "unindexed": [], "index_only": []}
    out: Dict[str, dict] = {}

    def add(path, names=None):
        hdr, _ = read_header(path)
        for name, e in hdr.items():
            if names is not None and name not in names:
                info["unindexed"].append(name)
                continue
            lo, hi = e["data_offsets"]
            out[name] = {"dtype": e["dtype"], "shape": tuple(int(v) for v in e["shape"]), "bytes": int(hi - lo), "file": os.path.basename(path)}
        if names is not None:
            info["index_only"].extend(sorted(set(names) - set(hdr)))

    if os.path.isfile(folder):
        add(folder)
        return out, info
    files = sorted(os.listdir(folder))
    idx = [f for f in files if f.endswith(".safetensors.index.json")]
    if idx:
        if len(idx) > 1:
            raise ValueError(f"{folder}: several index files {idx}")
        info["index"] = idx[0]
        with open(os.path.join(folder, idx[0])) as f:
            wm = json.load(f)["weight_map"]
        by_file: Dict[str, set] = {}
        for name, fn in wm.items():
            by_file.setdefault(fn, set()).add(name)
        for fn, names in sorted(by_file.items()):
            p = os.path.join(folder, fn)
            if not os.path.exists(p):
                info["missing_shards"].append(fn)
                continue
            add(p, names)
        return out, info
    st = [f for f in files if f.endswith(".safetensors")]
    if len(st) != 1:
        raise FileNotFoundError(f"{folder}: expected one *.safetensors file or an index, found {st}")
    add(os.path.join(folder, st[0]))
    return out, info


def compare_header(found: Dict[str, dict], expected: Dict[str, tuple], numel_only: Iterable[str] = ()) -> Tuple[List[str], List[str], List[dict]]:
    """-> (missing, unexpected, wrong_shape [{key, found, expected}]) of a header against {key: shape}; keys in `numel_only` (tensors
    the loader reshapes) are compared by element count."""
    loose = set(numel_only)
    missing = sorted(set(expected) - set(found))
    unexpected = sorted(set(found) - set(expected))
    wrong = []
    for k in sorted(set(found) & set(expected)):
        f, e = tuple(found[k]["shape"]), tuple(int(v) for v in expected[k])
        if (int(np.prod(f)) != int(np.prod(e))) if k in loose else (f != e):
            wrong.append({"key": k, "found": list(f), "expected": list(e)})
    return missing, unexpected, wrong


# ---- audit ---------------------------------------------------------------------------------------------------------------------------
def _component(kind: str, folder: str) -> dict:
    return {"kind": kind, "folder": folder, "missing": [], "unexpected": [], "wrong_shape": [], "dtypes": {}, "bytes": 0,
            "index": {"index": None, "missing_shards": [], "unindexed": [], "index_only": []}, "refused": [], "notes": []}


def _fill_header(c: dict, folder: str) -> Optional[Dict[str, dict]]:
    try:
        found, info = dir_header(folder)
    except (FileNotFoundError, ValueError, KeyError, json.JSONDecodeError) as e:
        c["notes"].append(f"unreadable: {e}")
        c["missing"].append("*.safetensors")
        return None
    c["index"] = info
    for e in found.values():
        c["dtypes"][e["dtype"]] = c["dtypes"].get(e["dtype"], 0) + 1
        c["bytes"] += e["bytes"]
    return found


def _read_json(path: str, c: dict) -> Optional[dict]:
    if not os.path.exists(path):
        c["notes"].append(f"{os.path.basename(path)} is absent")
        return None
    try:
        with open(path) as f:
            cj = json.load(f)
        if not isinstance(cj, dict):
            raise ValueError("not a JSON object")
        return cj
    except (ValueError, UnicodeDecodeError) as e:   # (json.JSONDecodeError is a ValueError)
        c["refused"].append(f"{os.path.basename(path)} is unreadable: {e}")
        return None


def _audit_longcat_dit(folder: str):
    from .longcat_dit import config_from_dict, expected_state_dict
    c = _component("LongCatVideoTransformer3DModel", folder)
    cj = _read_json(os.path.join(folder, "config.json"), c)
    cfg = None
    if cj is None:
        if not c["refused"]:
            c["missing"].append("config.json")
    else:
        try:
            cfg, _, ignored = config_from_dict(cj)
            if ignored:
                c["notes"].append(f"config keys the loader ignores: {ignored}")
        except ValueError as e:
            c["refused"].append(str(e))
    found = _fill_header(c, folder)
    if found is not None and cfg is not None:
        c["missing"], c["unexpected"], c["wrong_shape"] = compare_header(found, expected_state_dict(cfg))
    return c, cfg


def _audit_wan_dit(folder: str) -> dict:
    from .dit import config_from_diffusers, expected_diffusers_state_dict
    c = _component("WanTransformer3DModel", folder)
    cj = _read_json(os.path.join(folder, "config.json"), c)
    if cj is None:
        c["notes"].append("shapes are checked against the Wan2.1-I2V-14B defaults")
    elif cj.get("_class_name") not in (None, "WanTransformer3DModel"):
        c["refused"].append(f"_class_name is {cj.get('_class_name')!r}, the loader is WanTransformer3DModel")
    found = _fill_header(c, folder)
    if found is not None:
        c["missing"], c["unexpected"], c["wrong_shape"] = compare_header(
            found, expected_diffusers_state_dict(config_from_diffusers(cj or {})), numel_only=_wan_reshaped(found))
    return c


def _wan_reshaped(found) -> List[str]:
    """Wan DiT tensors the loader reshapes itself (patch embedding, modulation tables): compared by element count."""
    return [k for k in found if k == "patch_embedding.weight" or k.endswith("scale_shift_table")]


def _audit_vae(folder: str) -> dict:
    """Key coverage by vae.diffusers_key_map(): its module names, each with at least one parameter in the folder; the leaves the loader
    reads are .weight / .bias / .gamma.  Shapes are not checked (the loader holds no shape table of the diffusers layout)."""
    from .vae import diffusers_key_map
    c = _component("AutoencoderKLWan", folder)
    found = _fill_header(c, folder)
    if found is None:
        return c
    km = diffusers_key_map()
    seen = set()
    for k in sorted(found):
        base, _, leaf = k.rpartition(".")
        if base in km and leaf in ("weight", "bias", "gamma"):
            seen.add(base)
        else:
            c["unexpected"].append(k)
    c["missing"] = sorted(f"{b}.*" for b in set(km) - seen)
    c["notes"].append("shapes not checked")
    return c


def _audit_text_encoder(folder: str) -> dict:
    """umt5.UMT5EncoderModel.from_pretrained's header check: `decoder.*` / `lm_head.*` are noted, not counted; the tied
    `encoder.embed_tokens.weight` stands in for `shared.weight` when that is absent."""
    from .umt5 import UMT5Config, consumed_header, expected_state_dict
    c = _component("UMT5EncoderModel", folder)
    cj = _read_json(os.path.join(folder, "config.json"), c)
    cfg = None
    if cj is None:
        if not c["refused"]:
            c["missing"].append("config.json")
    else:
        try:
            cfg = UMT5Config.from_dict(cj)
        except (NotImplementedError, ValueError, TypeError) as e:
            c["refused"].append(str(e))
    found = _fill_header(c, folder)
    if found is not None and cfg is not None:
        keep, dropped = consumed_header(found)
        if dropped:
            c["notes"].append(f"{dropped} decoder.* / lm_head.* tensors are ignored by the encoder")
        c["missing"], c["unexpected"], c["wrong_shape"] = compare_header(keep, expected_state_dict(cfg))
    return c


def _audit_image_encoder(folder: str) -> dict:
    """clip.CLIPVisionModel.from_pretrained's header check: keys with or without the `vision_model.` prefix; the text tower and the
    projections of a full CLIPModel file are noted, not counted; the last layer and post_layernorm are checked though never uploaded."""
    from .clip import CLIPVisionConfig, consumed_header, expected_state_dict
    c = _component("CLIPVisionModel", folder)
    cj = _read_json(os.path.join(folder, "config.json"), c)
    cfg = None
    if cj is None:
        if not c["refused"]:
            c["missing"].append("config.json")
    else:
        try:
            cfg = CLIPVisionConfig.from_dict(cj)
        except (NotImplementedError, ValueError, TypeError) as e:
            c["refused"].append(str(e))
    found = _fill_header(c, folder)
    if found is not None and cfg is not None:
        keep, dropped, _ = consumed_header(found)
        if dropped:
            c["notes"].append(f"{dropped} text_model.* / projection / logit_scale tensors are ignored by the vision encoder")
        c["missing"], c["unexpected"], c["wrong_shape"] = compare_header(keep, expected_state_dict(cfg))
    return c


_SCHED_VALUES = ("shift", "flow_shift", "num_train_timesteps", "prediction_type", "solver_order")


def _audit_scheduler(folder: str, longcat: bool) -> dict:
    """The values that decide the schedule, and every flag the scheduler class of this engine refuses (its constructor raises
    NotImplementedError): found by handing the file to that constructor, which computes a few scalars on the host."""
    c = _component("FlowMatchEulerDiscreteScheduler" if longcat else "UniPCMultistepScheduler", folder)
    cj = _read_json(os.path.join(folder, "scheduler_config.json"), c)
    if cj is None:
        if not c["refused"]:
            c["missing"].append("scheduler_config.json")
        return c
    c["values"] = {k: cj[k] for k in _SCHED_VALUES if k in cj}
    name = cj.get("_class_name")
    if name is not None:
        c["values"]["_class_name"] = name
        longcat = "FlowMatch" in name if ("FlowMatch" in name or "UniPC" in name) else longcat
        c["kind"] = "FlowMatchEulerDiscreteScheduler" if longcat else "UniPCMultistepScheduler"
    if longcat:
        from .longcat_scheduler import FlowMatchEulerDiscreteScheduler as cls
        flags = ("use_dynamic_shifting", "invert_sigmas", "shift_terminal", "use_karras_sigmas", "use_exponential_sigmas",
                 "use_beta_sigmas", "stochastic_sampling")
        bad = [f"{k}={cj[k]!r}" for k in flags if cj.get(k)]
    else:
        from .scheduler import UniPCMultistepScheduler as cls
        want = dict(prediction_type="flow_prediction", use_flow_sigmas=True, predict_x0=True, solver_type="bh2", solver_order=2,
                    final_sigmas_type="zero")
        bad = [f"{k}={cj[k]!r}" for k, v in want.items() if k in cj and cj[k] != v]
    try:
        cls.from_config(cj)
    except NotImplementedError as e:   # the constructor is the rule; the flag names above only say which setting it was
        c["refused"] = bad or [str(e)]
    return c


_LORA_H = "___lorahyphen___"


def _audit_lora(path: str, expected: Optional[Dict[str, tuple]]) -> dict:
    """longcat_dit._lora_target / _parse_lora restated on shapes: every `<name>.lora_down.weight` must name a Linear of the model
    (a 2-D `<module>.weight` of expected_state_dict), its down-projection is [nsep * rank, K] and its nsep up-projections
    [rows / nsep, rank] for the Linear's [rows, K].  `unexpected`: entries without a Linear (and tensors that belong to no entry);
    `missing`: entries without an up-projection; `wrong_shape`: the rest."""
    c = _component("LoRA", path)
    found = _fill_header(c, path)
    if found is None:
        return c
    if expected is None:
        c["notes"].append("no readable dit/ beside it: entries not resolved")
        return c
    used = set()
    for key in sorted(found):
        if not key.endswith(".lora_down.weight"):
            continue
        name = key[: -len(".lora_down.weight")]
        module = name.replace("lora" + _LORA_H, "").replace(_LORA_H, ".")
        used.add(key)
        if name + ".alpha_scale" in found:
            used.add(name + ".alpha_scale")
        ups = [name + ".lora_up.weight"] if name + ".lora_up.weight" in found else \
            sorted((k for k in found if k.startswith(name + ".lora_up.blocks.")), key=lambda k: int(k.split(".")[-2]))
        used.update(ups)
        shape = expected.get(module + ".weight")
        if shape is None or len(shape) != 2:
            c["unexpected"].append(key)
            continue
        if not ups:
            c["missing"].append(name + ".lora_up.weight")
            continue
        rows, K = shape
        down = found[key]["shape"]
        nsep = len(ups)
        rank = down[0] // nsep if len(down) == 2 else 0
        ok = (len(down) == 2 and down[1] == K and rank > 0 and down[0] == nsep * rank and rows % nsep == 0
              and all(tuple(found[u]["shape"]) == (rows // nsep, rank) for u in ups))
        if not ok:
            c["wrong_shape"].append({"key": key, "found": {"down": list(down), "up": [list(found[u]["shape"]) for u in ups]},
                                     "expected": {"linear": [rows, K]}})
    c["unexpected"].extend(sorted(set(found) - used))
    return c


def audit(path: str) -> dict:
    """What the loaders of this engine would find in the checkpoint folder `path`: {"path", "components": {name: report}, "ok"}.
    Every report has `missing`, `unexpected`, `wrong_shape`, `dtypes` (count per dtype), `bytes`, `index` (shards the index names
    that are absent, tensors outside the index), `refused` (settings a class of this engine raises on) and `notes`; the scheduler's
    also `values`.  ok = at least one component found, nothing missing, unexpected, mis-shaped or refused, no shard absent and no tensor
    that the index lists but its shard lacks.  Tensors that a shard holds and the index does not list (`index.unindexed`) are REPORTED
    ONLY: load_dir never reads them, so they do not stand in the way of loading."""
    if not os.path.isdir(path):
        raise FileNotFoundError(f"checkpoint folder does not exist: {path}")
    comps: Dict[str, dict] = {}
    expected = None
    if os.path.isdir(os.path.join(path, "dit")):
        from .longcat_dit import expected_state_dict
        comps["dit"], cfg = _audit_longcat_dit(os.path.join(path, "dit"))
        expected = expected_state_dict(cfg) if cfg is not None else None
    if os.path.isdir(os.path.join(path, "transformer")):
        comps["transformer"] = _audit_wan_dit(os.path.join(path, "transformer"))
    if os.path.isdir(os.path.join(path, "vae")):
        comps["vae"] = _audit_vae(os.path.join(path, "vae"))
    if os.path.isdir(os.path.join(path, "text_encoder")):
        comps["text_encoder"] = _audit_text_encoder(os.path.join(path, "text_encoder"))
    if os.path.isdir(os.path.join(path, "image_encoder")):
        comps["image_encoder"] = _audit_image_encoder(os.path.join(path, "image_encoder"))
    if os.path.isdir(os.path.join(path, "scheduler")):
        comps["scheduler"] = _audit_scheduler(os.path.join(path, "scheduler"), longcat="dit" in comps or "transformer" not in comps)
    for f in sorted(glob.glob(os.path.join(path, "lora", "*.safetensors"))):
        comps["lora/" + os.path.splitext(os.path.basename(f))[0]] = _audit_lora(f, expected)
    ok = bool(comps) and not any(c["missing"] or c["unexpected"] or c["wrong_shape"] or c["refused"] or c["index"]["missing_shards"]
                                 or c["index"]["index_only"] for c in comps.values())
    return {"path": path, "components": comps, "ok": ok}


def audit_vggt(folder: str, depth: bool = True) -> dict:
    """vggt.VGGT.from_pretrained(folder, depth=depth)'s header check as a report of the same form as `audit` (headers and config.json only,
    no GPU): the one component is `vggt`; the heads this engine does not run (point, track) are noted, not counted."""
    from .vggt import VGGTConfig, consumed_header, expected_state_dict
    if not os.path.isdir(folder):
        raise FileNotFoundError(f"checkpoint folder does not exist: {folder}")
    c = _component("VGGT", folder)
    cfg = None
    cj = os.path.join(folder, "config.json")
    if os.path.exists(cj):
        d = _read_json(cj, c)
        if d is not None:
            try:
                cfg = VGGTConfig.from_dict(d)
                if depth:
                    cfg.check_depth_layers()
            except (NotImplementedError, ValueError, TypeError, KeyError) as e:
                c["refused"].append(str(e))
    else:
        c["notes"].append("config.json is absent: the released configuration is assumed")
        cfg = VGGTConfig()
    path = os.path.join(folder, "model.safetensors")
    found = None
    if not os.path.exists(path):
        c["missing"].append("model.safetensors")
    else:
        try:
            found, _ = read_header(path)
        except (ValueError, KeyError, json.JSONDecodeError, OSError) as e:
            c["notes"].append(f"unreadable: {e}")
            c["missing"].append("model.safetensors")
    if found is not None:
        for e in found.values():
            c["dtypes"][e["dtype"]] = c["dtypes"].get(e["dtype"], 0) + 1
            c["bytes"] += int(e["data_offsets"][1] - e["data_offsets"][0])
        if cfg is not None and not c["refused"]:
            shapes = {k: {"shape": tuple(int(v) for v in e["shape"])} for k, e in found.items()}
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", UserWarning)  # (the loader's one warning is the note below)
                keep = consumed_header(shapes, folder, depth)
            if len(keep) < len(shapes):
                c["notes"].append(f"{len(shapes) - len(keep)} tensors of heads this engine does not run are ignored")
            c["missing"], c["unexpected"], c["wrong_shape"] = compare_header(keep, expected_state_dict(cfg, depth))
    ok = not (c["missing"] or c["unexpected"] or c["wrong_shape"] or c["refused"])
    return {"path": folder, "components": {"vggt": c}, "ok": ok}


def format_report(rep: dict, limit: int = 10) -> str:
    """The text report: per component the counts and at most `limit` names per class."""
    lines = [f"checkpoint {rep['path']}: {'OK' if rep['ok'] else 'PROBLEMS'}"]
    if not rep["components"]:
        lines.append("  no component folder found (dit/, transformer/, vae/, text_encoder/, image_encoder/, scheduler/, lora/*.safetensors)")
    for name, c in rep["components"].items():
        dt = ", ".join(f"{k} x {v}" for k, v in sorted(c["dtypes"].items())) or "-"
        lines.append(f"  {name} ({c['kind']}): {sum(c['dtypes'].values())} tensors, {c['bytes'] / 2 ** 30:.3f} GiB, dtypes {dt}")
        if c.get("values"):
            lines.append("    values: " + ", ".join(f"{k}={v!r}" for k, v in c["values"].items()))
        classes = [("missing", c["missing"]), ("unexpected", c["unexpected"]),
                   ("wrong_shape", [f"{w['key']}: found {w['found']}, expected {w['expected']}" for w in c["wrong_shape"]]),
                   ("refused", c["refused"]), ("missing shards", c["index"]["missing_shards"]),
                   ("in a shard but not in the index", c["index"]["unindexed"]), ("in the index but not in its shard", c["index"]["index_only"])]
        for label, items in classes:
            if items:
                more = f" ... and {len(items) - limit} more" if len(items) > limit else ""
                lines.append(f"    {label}: {len(items)}")
                lines.extend(f"      {it}" for it in items[:limit])
                if more:
                    lines.append("     " + more)
        lines.extend(f"    note: {n}" for n in c["notes"])
    return "\n".join(lines)


def main(argv=None) -> int:
    import argparse
    ap = argparse.ArgumentParser(prog="python -m worldforge_amd.checkpoint",
                                 description="Audit a checkpoint folder against this engine's loaders (headers and JSON only, no GPU)")
    ap.add_argument("path")
    ap.add_argument("--json", action="store_true", help="print the report as JSON")
    ap.add_argument("--vggt", action="store_true", help="the folder is a VGGT checkpoint (model.safetensors with the depth head), as run_warp takes it")
    a = ap.parse_args(argv)
    rep = audit_vggt(a.path, depth=True) if a.vggt else audit(a.path)
    print(json.dumps(rep, indent=1) if a.json else format_report(rep))
    return 0 if rep["ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
