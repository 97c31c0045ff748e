"""Pooling defaults of an embedding checkpoint.

sentence-transformers checkpoints describe what follows the transformer in
two files of the model directory: modules.json (the module chain: Transformer,
Pooling, optionally Normalize or Dense) and 1_Pooling/config.json (which
pooling). The engine pools by last token, mean or first token and can L2
normalise; a checkpoint that asks for anything else fails the load, naming the
setting, because the alternative is serving vectors that are silently wrong.
"""

from __future__ import annotations

import json
import os

_MODES = {
    "pooling_mode_lasttoken": "last",
    "pooling_mode_mean_tokens": "mean",
    "pooling_mode_cls_token": "cls",
}
_UNSUPPORTED = (
    "pooling_mode_max_tokens",
    "pooling_mode_mean_sqrt_len_tokens",
    "pooling_mode_weightedmean_tokens",
)


def _read_json(path: str):
    with open(path) as f:
        return json.load(f)


def read_st_pooling(model_path: str | None) -> dict | None:
    """{"mode", "normalize"} from the sentence-transformers files under
    model_path, None when it has no modules.json. ValueError for settings
    the engine cannot honour."""
    if not model_path:
        return None
    mpath = os.path.join(model_path, "modules.json")
    if not os.path.exists(mpath):
        return None
    modules = _read_json(mpath)
    normalize = False
    pooling_dir = None
    for m in modules:
        kind = str(m.get("type", "")).rsplit(".", 1)[-1]
        if kind == "Transformer":
            continue
        if kind == "Pooling":
            pooling_dir = m.get("path", "1_Pooling")
        elif kind == "Normalize":
            normalize = True
        else:
            raise ValueError(
                f"{mpath}: unsupported sentence-transformers module "
                f"{m.get('type')!r} ({kind} is not implemented; supported: "
                "Transformer, Pooling, Normalize)")
    if pooling_dir is None:
        raise ValueError(f"{mpath}: no Pooling module")
    cpath = os.path.join(model_path, pooling_dir, "config.json")
    if not os.path.exists(cpath):
        raise ValueError(f"{mpath} names a Pooling module but {cpath} is missing")
    pc = _read_json(cpath)
    for key in _UNSUPPORTED:
        if pc.get(key):
            raise ValueError(
                f"{cpath}: unsupported pooling {key}=true (supported: "
                f"{', '.join(_MODES)})")
    if pc.get("include_prompt", True) is False:
        raise ValueError(
            f"{cpath}: unsupported include_prompt=false (prompt tokens "
            "cannot be excluded from pooling)")
    on = [mode for key, mode in _MODES.items() if pc.get(key)]
    if len(on) != 1:
        raise ValueError(
            f"{cpath}: exactly one of {', '.join(_MODES)} must be true "
            f"(concatenated poolings are unsupported), got {on or 'none'}")
    return {"mode": on[0], "normalize": normalize}


def resolve_default_pooling(model_path: str | None, pooling: str = "auto",
                            normalize: str = "auto") -> dict:
    """Default pooling spec of an engine: explicit settings win, then the
    checkpoint's sentence-transformers files, then last token + normalise.
    The files are validated even when both settings are explicit."""
    if pooling not in ("auto", "last", "mean", "cls"):
        raise ValueError(
            f"pooling must be auto, last, mean or cls, got {pooling!r}")
    normalize = str(normalize).lower()
    if normalize not in ("auto", "true", "false"):
        raise ValueError(
            f"embedding_normalize must be auto, true or false, got {normalize!r}")
    st = read_st_pooling(model_path) or {"mode": "last", "normalize": True}
    return {
        "mode": st["mode"] if pooling == "auto" else pooling,
        "normalize": (st["normalize"] if normalize == "auto"
                      else normalize == "true"),
        "dims": None,
    }
