"""Embedding requests on the CPU: ops.ref.pool_embed against an fp64 oracle,
model parity with transformers, the engine's handling of pooling sequences
and the sentence-transformers settings reader."""

import json
import os

import numpy as np
import pytest
import torch

import arks_amd.ops as ops
from arks_amd.config import PRESET_CONFIGS, EngineConfig, ModelConfig
from arks_amd.engine import LLMEngine, SamplingParams
from arks_amd.loader.pooling_config import (read_st_pooling,
                                            resolve_default_pooling)
from embed_testutil import (EPS, HIDDENS, MODES, SEG_LENS, dims_for,
                            make_inputs, oracle_all, run_mean_chunked,
                            whole_segments)

# CPU fp32 reference against the fp64 oracle: the largest difference measured
# on these inputs is 8.8e-8 over every case
REF_ATOL = 1e-6


def cpu_pool(H, entries, carry, dims, normalize=True):
    x, residual, weight, _ = make_inputs(H)
    return ops.pool_embed(x, residual, weight, EPS,
                          ops.build_pool_table(entries), carry, dims=dims,
                          normalize=normalize)


@pytest.mark.parametrize("H", HIDDENS)
@pytest.mark.parametrize("mode", MODES)
def test_ref_matches_fp64_oracle(H, mode):
    for dims in dims_for(H):
        got = cpu_pool(H, whole_segments(H, mode), None, dims)
        assert got.shape == (len(SEG_LENS), dims) and got.dtype == torch.float32
        want = oracle_all(H, mode, dims)
        assert (got.double() - want).abs().max().item() <= REF_ATOL


@pytest.mark.parametrize("H", HIDDENS)
def test_ref_mean_through_the_carry(H):
    for dims in dims_for(H):
        got = run_mean_chunked(lambda e, c: cpu_pool(H, e, c, dims), H, dims,
                               "cpu")
        want = oracle_all(H, "mean", dims)
        assert (got.double() - want).abs().max().item() <= REF_ATOL


def test_pool_table_and_argument_checks():
    x = torch.zeros(8, 16, dtype=torch.bfloat16)
    w = torch.ones(16, dtype=torch.bfloat16)
    ok = ops.build_pool_table([(0, 8, "mean", -1, 0, 1)])
    for dims in (0, 17):
        with pytest.raises(ValueError, match="dims"):
            ops.pool_embed(x, x, w, EPS, ok, None, dims=dims)
    with pytest.raises(ValueError, match="H % 8"):
        ops.pool_embed(x[:, :12], x[:, :12], w[:12], EPS, ok, None)
    with pytest.raises(ValueError, match="row"):
        ops.pool_embed(x, x, w, EPS,
                       ops.build_pool_table([(6, 3, "last", -1, 0, 1)]), None)
    with pytest.raises(ValueError, match="slot"):  # a carry needs a slot
        ops.build_pool_table([(0, 4, "mean", -1, 0, 0)])
    with pytest.raises(ValueError, match="slot"):  # and its own
        ops.build_pool_table([(0, 4, "mean", 0, 0, 0), (4, 4, "mean", 0, 4, 1)])
    with pytest.raises(ValueError, match="carry"):
        ops.pool_embed(x, x, w, EPS,
                       ops.build_pool_table([(0, 4, "mean", 2, 0, 0)]),
                       torch.zeros(2, 16))
    with pytest.raises(KeyError):
        ops.build_pool_table([(0, 4, "max", -1, 0, 1)])


# --------------------------- model parity ---------------------------------
PARITY_PROMPTS = [[1, 17, 300, 42, 42, 7, 99, 123, 8, 55, 4],
                  [9, 8, 7, 6, 5],
                  [(7 * i + 3) % 500 + 1 for i in range(37)]]


def _fp32_engine(**kw):
    base = dict(device="cpu", kv_cache_blocks=256, max_model_len=512,
                max_num_seqs=16, dtype="float32")
    base.update(kw)
    return LLMEngine(EngineConfig(**base))


def _as_base_model(src: str, dst: str, arch: str):
    """Re-save a ...ForCausalLM checkpoint as its base model: tensor names
    without `model.`, no lm_head, embeddings not tied."""
    from safetensors.torch import load_file, save_file

    os.makedirs(dst)
    tensors = load_file(os.path.join(src, "model.safetensors"))
    save_file({k.removeprefix("model."): v for k, v in tensors.items()
               if not k.startswith("lm_head.")},
              os.path.join(dst, "model.safetensors"))
    with open(os.path.join(src, "config.json")) as f:
        cfg = json.load(f)
    cfg.update(architectures=[arch], tie_word_embeddings=False)
    with open(os.path.join(dst, "config.json"), "w") as f:
        json.dump(cfg, f)


def test_embeddings_match_transformers(tmp_path):
    transformers = pytest.importorskip("transformers")
    from arks_amd.loader.safetensors_loader import save_random_checkpoint

    cfg = PRESET_CONFIGS["tiny-qwen3"]
    causal = str(tmp_path / "causal")
    save_random_checkpoint(cfg, causal, seed=7)
    hf_cfg = transformers.Qwen3Config(
        vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size,
        intermediate_size=cfg.intermediate_size,
        num_hidden_layers=cfg.num_hidden_layers,
        num_attention_heads=cfg.num_attention_heads,
        num_key_value_heads=cfg.num_key_value_heads, head_dim=cfg.head_dim,
        rms_norm_eps=cfg.rms_norm_eps, rope_theta=cfg.rope_theta,
        max_position_embeddings=cfg.max_position_embeddings,
        tie_word_embeddings=cfg.tie_word_embeddings, attention_bias=False,
        attention_dropout=0.0)
    hf = transformers.Qwen3Model.from_pretrained(
        causal, config=hf_cfg, torch_dtype=torch.float32).eval()
    want = {m: [] for m in MODES}
    with torch.no_grad():
        for p in PARITY_PROMPTS:
            h = hf(torch.tensor([p])).last_hidden_state[0]
            for m, v in (("last", h[-1]), ("mean", h.mean(0)), ("cls", h[0])):
                want[m].append(torch.nn.functional.normalize(v, dim=0).numpy())

    engine = _fp32_engine(model_path=causal)
    base = str(tmp_path / "base")
    _as_base_model(causal, base, "Qwen3Model")
    embedder = _fp32_engine(model_path=base)
    assert engine.can_generate and not embedder.can_generate
    assert embedder.model_cfg.qk_norm  # Qwen3Model maps to Qwen3's behaviour
    for m in MODES:
        got = engine.embed(PARITY_PROMPTS, {"mode": m})
        same = embedder.embed(PARITY_PROMPTS, {"mode": m})
        for g, s, w in zip(got, same, want[m]):
            assert np.abs(g - w).max() < 2e-3  # the fp32 parity bound
            assert np.array_equal(g, s)
    # no lm_head: generation is refused, never sampled from an empty head
    with pytest.raises(ValueError, match="embedding"):
        embedder.generate([[1, 2, 3]], SamplingParams(max_tokens=2))
    assert not embedder.has_work()


def test_base_model_architectures_map_to_their_causal_lm():
    q2 = ModelConfig.from_hf_config({"architectures": ["Qwen2Model"]})
    assert q2.architecture == "Qwen2ForCausalLM" and q2.attention_bias
    assert not q2.qk_norm
    q3 = ModelConfig.from_hf_config({"architectures": ["Qwen3Model"]})
    assert q3.qk_norm and not q3.attention_bias
    for arch in ("MistralModel", "LlamaModel"):
        c = ModelConfig.from_hf_config({"architectures": [arch]})
        assert c.architecture == arch[:-5] + "ForCausalLM"
        assert not c.attention_bias and not c.qk_norm


# --------------------------- engine behaviour ------------------------------
LONG = [(11 * i + 5) % 500 + 1 for i in range(50)]
BATCH = [LONG, [1, 5, 9, 20, 31, 7], [3, 3, 7, 90], [44]]


@pytest.fixture(scope="module")
def whole():
    return _fp32_engine(preset="tiny")


@pytest.mark.parametrize("mode", MODES)
def test_chunked_prefill_gives_the_same_vectors(whole, mode):
    chunked = _fp32_engine(preset="tiny", max_num_batched_tokens=16)
    steps = 0
    seqs = [chunked.add_request(p, pooling={"mode": mode}) for p in BATCH]
    while chunked.has_work():
        chunked.step()
        steps += 1
    assert steps >= 4  # the 50-token prompt alone spans four chunks
    want = whole.embed(BATCH, {"mode": mode})
    for s, w in zip(seqs, want):
        assert s.num_output_tokens == 0 and s.finish_reason == "stop"
        assert np.abs(s.embedding - w).max() <= 1e-5
    assert not chunked.runner._pool_slots


def test_prefix_cache_serves_last_but_not_mean_or_cls():
    e = _fp32_engine(preset="tiny")
    free0 = e.scheduler.allocator.num_free
    first = e.embed([LONG], {"mode": "last"})[0]
    hits = e.prefix_cache_stats[0]
    again = e.embed([LONG], {"mode": "last"})[0]
    assert e.prefix_cache_stats[0] == hits + 48  # three full pages of 16
    assert np.abs(again - first).max() <= 1e-5
    for mode in ("mean", "cls"):
        hits = e.prefix_cache_stats[0]
        e.embed([LONG], {"mode": mode})
        assert e.prefix_cache_stats[0] == hits
    assert e.scheduler.allocator.num_free == free0
    assert not e.scheduler.running and not e.scheduler.waiting


def test_generation_next_to_pooling_is_unchanged():
    sp = SamplingParams(max_tokens=8, ignore_eos=True)
    gen_prompts = [[1, 5, 9, 20, 31, 7], LONG[:30]]
    alone = _fp32_engine(preset="tiny", max_num_batched_tokens=32).generate(
        gen_prompts, sp)
    e = _fp32_engine(preset="tiny", max_num_batched_tokens=32)
    free0 = e.scheduler.allocator.num_free
    gen = [e.add_request(gen_prompts[0], sp)]
    emb = [e.add_request(LONG, pooling={"mode": "mean"})]
    gen.append(e.add_request(gen_prompts[1], sp))
    emb.append(e.add_request([3, 3, 7, 90], pooling={"mode": "last",
                                                     "dims": 40}))
    for _ in range(3):
        e.step()
    # joins while the others decode: a mixed batch
    emb.append(e.add_request(LONG[:45], pooling={"mode": "cls",
                                                 "normalize": False}))
    outs = []
    while e.has_work():
        outs += e.step()
    assert [s.output_token_ids for s in gen] == alone
    assert [s.embedding.shape for s in emb] == [(128,), (40,), (128,)]
    done = [o for o in outs if o.embedding is not None]
    assert all(o.finished and o.new_token_id == -1
               and o.num_output_tokens == 0 for o in done)
    assert e.scheduler.allocator.num_free == free0
    assert e.total_output_tokens == 16


def test_pooling_completes_under_ngram_speculation(whole):
    e = _fp32_engine(preset="tiny", speculative="ngram")
    sp = SamplingParams(max_tokens=12, ignore_eos=True)
    g = e.add_request([5, 6, 7, 5, 6, 7, 5, 6], sp)
    e.step()
    seqs = [e.add_request(p, pooling={"mode": "mean"}) for p in BATCH]
    while e.has_work():
        e.step()
    assert len(g.output_token_ids) == 12
    want = whole.embed(BATCH, {"mode": "mean"})
    for s, w in zip(seqs, want):
        assert np.abs(s.embedding - w).max() <= 1e-5


def _first_token_agrees(engine, prompts):
    emb = engine.embed(prompts, {"mode": "last", "normalize": False})
    first = engine.generate(prompts, SamplingParams(max_tokens=1))
    head = engine.runner.model.lm_head.weight.float()
    V = engine.model_cfg.vocab_size
    return [int((head[:V] @ torch.from_numpy(e)).argmax()) == f[0]
            for e, f in zip(emb, first)]


def test_last_embedding_predicts_the_first_greedy_token(whole):
    """Without normalisation e_last is the row generation samples from."""
    assert all(_first_token_agrees(whole, BATCH))
    # the eight prompts of the GPU engine test, on its preset, in fp32
    from embed_testutil import ENGINE_PROMPTS as PROMPTS

    e = _fp32_engine(preset="tiny-gpu", max_model_len=1024,
                     max_num_batched_tokens=64)
    assert all(_first_token_agrees(e, PROMPTS))


def test_pooling_spec_is_validated(whole):
    for bad in ({"mode": "max"}, {"dims": 0}, {"dims": 129}, {"dims": 1.5},
                {"weights": 1}):
        with pytest.raises(ValueError):
            whole.add_request([1, 2, 3], pooling=bad)
    with pytest.raises(ValueError):
        whole.add_request([], pooling={"mode": "last"})
    assert not whole.has_work()


# ------------------- sentence-transformers settings -------------------------
ST = "sentence_transformers.models."


def _st_dir(root, modules, pooling=None):
    os.makedirs(root / "1_Pooling", exist_ok=True)
    (root / "modules.json").write_text(json.dumps([
        {"idx": i, "name": str(i), "path": "" if m == "Transformer"
         else f"{i}_{m}", "type": ST + m} for i, m in enumerate(modules)]))
    if pooling is not None:
        base = {"word_embedding_dimension": 128, "pooling_mode_cls_token": False,
                "pooling_mode_mean_tokens": False,
                "pooling_mode_max_tokens": False,
                "pooling_mode_mean_sqrt_len_tokens": False,
                "pooling_mode_weightedmean_tokens": False,
                "pooling_mode_lasttoken": False, "include_prompt": True}
        base.update(pooling)
        (root / "1_Pooling" / "config.json").write_text(json.dumps(base))
    return str(root)


@pytest.mark.parametrize("key,mode", [("pooling_mode_lasttoken", "last"),
                                      ("pooling_mode_mean_tokens", "mean"),
                                      ("pooling_mode_cls_token", "cls")])
@pytest.mark.parametrize("normalize", [True, False])
def test_st_settings_give_the_defaults(tmp_path, key, mode, normalize):
    mods = ["Transformer", "Pooling"] + (["Normalize"] if normalize else [])
    path = _st_dir(tmp_path, mods, {key: True})
    assert read_st_pooling(path) == {"mode": mode, "normalize": normalize}
    assert resolve_default_pooling(path) == {
        "mode": mode, "normalize": normalize, "dims": None}
    # explicit settings win over the files
    assert resolve_default_pooling(path, "cls", "true") == {
        "mode": "cls", "normalize": True, "dims": None}


def test_no_st_files_means_last_and_normalize(tmp_path):
    assert read_st_pooling(str(tmp_path)) is None
    assert resolve_default_pooling(str(tmp_path)) == {
        "mode": "last", "normalize": True, "dims": None}
    assert resolve_default_pooling(None, "mean", "false") == {
        "mode": "mean", "normalize": False, "dims": None}
    with pytest.raises(ValueError, match="pooling"):
        resolve_default_pooling(None, "max")


@pytest.mark.parametrize("setting", [
    "pooling_mode_max_tokens", "pooling_mode_weightedmean_tokens",
    "pooling_mode_mean_sqrt_len_tokens"])
def test_unsupported_pooling_fails_the_load_by_name(tmp_path, setting):
    path = _st_dir(tmp_path, ["Transformer", "Pooling"], {setting: True})
    with pytest.raises(ValueError, match=setting):
        resolve_default_pooling(path, "last", "true")  # even when overridden


def test_unsupported_st_modules_and_options_fail_by_name(tmp_path):
    path = _st_dir(tmp_path / "dense", ["Transformer", "Pooling", "Dense"],
                   {"pooling_mode_lasttoken": True})
    with pytest.raises(ValueError, match="Dense"):
        read_st_pooling(path)
    path = _st_dir(tmp_path / "prompt", ["Transformer", "Pooling"],
                   {"pooling_mode_mean_tokens": True, "include_prompt": False})
    with pytest.raises(ValueError, match="include_prompt"):
        read_st_pooling(path)
    path = _st_dir(tmp_path / "two", ["Transformer", "Pooling"],
                   {"pooling_mode_mean_tokens": True,
                    "pooling_mode_cls_token": True})
    with pytest.raises(ValueError, match="exactly one"):
        read_st_pooling(path)


def test_engine_takes_its_defaults_from_the_checkpoint(tmp_path):
    from arks_amd.loader.safetensors_loader import save_random_checkpoint

    path = str(tmp_path)
    save_random_checkpoint(PRESET_CONFIGS["tiny"], path, seed=3)
    _st_dir(tmp_path, ["Transformer", "Pooling"],
            {"pooling_mode_mean_tokens": True})
    e = _fp32_engine(model_path=path)
    assert e.default_pooling == {"mode": "mean", "normalize": False,
                                 "dims": None}
    v = e.embed([LONG])[0]
    assert np.abs(v - e.embed([LONG], {"mode": "mean",
                                       "normalize": False})[0]).max() == 0
    assert abs(np.linalg.norm(v) - 1.0) > 1e-3  # not normalised
    _st_dir(tmp_path, ["Transformer", "Pooling", "Dense"],
            {"pooling_mode_mean_tokens": True})
    with pytest.raises(ValueError, match="Dense"):
        _fp32_engine(model_path=path)
