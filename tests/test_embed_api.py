"""POST /v1/embeddings on the engine server (CPU, tiny model, LoRA adapters
next to the base model) and through the gateway."""

import asyncio
import base64

import httpx
import numpy as np
import pytest

from arks_amd.controlplane import Operator, Store
from arks_amd.crd.types import parse_manifest
from arks_amd.gateway.app import create_gateway_app
from arks_amd.server.api import MAX_EMBEDDING_INPUTS, create_app
from arks_amd.server.async_engine import AsyncEngine
from arks_amd.server.tokenizer import ByteTokenizer
from lora_testutil import engine_cfg, make_adapters

TOKENS = [1, 5, 9, 20, 31, 7]


def make_app(tmp_path, disagg=None, **kw):
    cfg = engine_cfg("tiny", "cpu", served_model_name="tiny",
                     enable_lora=True, dtype="float32",
                     lora_modules=make_adapters("tiny", tmp_path), **kw)
    engine = AsyncEngine(cfg, model_name="tiny")
    mc = cfg.model_config()
    return create_app(engine, "tiny",
                      ByteTokenizer(mc.vocab_size, mc.eos_token_id),
                      disagg_mode=disagg)


@pytest.fixture()
def app(tmp_path):
    return make_app(tmp_path)


def run_with_client(app, fn):
    async def go():
        async with app.router.lifespan_context(app):
            transport = httpx.ASGITransport(app=app)
            async with httpx.AsyncClient(
                transport=transport, base_url="http://t", timeout=60
            ) as client:
                await fn(client)

    asyncio.new_event_loop().run_until_complete(go())


async def embed(client, **body):
    r = await client.post("/v1/embeddings", json={"model": "tiny", **body})
    assert r.status_code == 200, r.text
    return r.json()


def vec(item):
    return np.asarray(item["embedding"], dtype=np.float32)


def test_every_input_form_and_the_response_shape(app):
    async def fn(client):
        tok = app.state.tokenizer
        one = await embed(client, input="hello world")
        assert one["object"] == "list" and one["model"] == "tiny"
        assert [d["object"] for d in one["data"]] == ["embedding"]
        assert one["data"][0]["index"] == 0
        n = len(tok.encode("hello world"))
        assert one["usage"] == {"prompt_tokens": n, "total_tokens": n}
        v = vec(one["data"][0])
        assert v.shape == (128,) and abs(np.linalg.norm(v) - 1) < 1e-5

        batch = await embed(client, input=["hello world", "bye", "hello world"],
                            user="someone")
        assert [d["index"] for d in batch["data"]] == [0, 1, 2]
        assert np.abs(vec(batch["data"][0]) - v).max() < 1e-5
        assert np.abs(vec(batch["data"][2]) - v).max() < 1e-5
        assert np.abs(vec(batch["data"][1]) - v).max() > 1e-3
        m = 2 * n + len(tok.encode("bye"))
        assert batch["usage"] == {"prompt_tokens": m, "total_tokens": m}

        # token ids: one item, and nested, equal to the string they encode
        ids = tok.encode("hello world")
        flat = await embed(client, input=ids)
        assert len(flat["data"]) == 1
        assert flat["usage"]["prompt_tokens"] == n
        assert np.abs(vec(flat["data"][0]) - v).max() < 1e-5
        nested = await embed(client, input=[ids, TOKENS])
        assert len(nested["data"]) == 2
        assert nested["usage"]["prompt_tokens"] == n + len(TOKENS)
        assert np.abs(vec(nested["data"][0]) - v).max() < 1e-5

    run_with_client(app, fn)


def test_base64_and_dimensions(app):
    async def fn(client):
        full = vec((await embed(client, input=[TOKENS]))["data"][0])
        b64 = await embed(client, input=[TOKENS], encoding_format="base64")
        raw = base64.b64decode(b64["data"][0]["embedding"])
        assert len(raw) == 4 * 128
        assert np.array_equal(np.frombuffer(raw, dtype="<f4"), full)
        cut = vec((await embed(client, input=[TOKENS],
                               dimensions=48))["data"][0])
        assert cut.shape == (48,)
        want = full[:48] / np.linalg.norm(full[:48])
        assert np.abs(cut - want).max() < 1e-6
        both = await embed(client, input=[TOKENS], dimensions=33,
                           encoding_format="base64")
        got = np.frombuffer(base64.b64decode(both["data"][0]["embedding"]),
                            dtype="<f4")
        assert np.abs(got - full[:33] / np.linalg.norm(full[:33])).max() < 1e-6

    run_with_client(app, fn)


def test_bad_requests_are_400(app):
    async def fn(client):
        async def status(**body):
            r = await client.post("/v1/embeddings",
                                  json={"model": "tiny", **body})
            return r.status_code, r.text

        for body in (
            {"input": ""}, {"input": []}, {"input": ["ok", ""]},
            {"input": [[1, 2], []]},
            {"input": ["x"] * (MAX_EMBEDDING_INPUTS + 1)},
            {"input": [TOKENS], "dimensions": 0},
            {"input": [TOKENS], "dimensions": 129},
            {"input": [[1, 2, 512]]},  # outside the vocabulary
        ):
            code, text = await status(**body)
            assert code == 400, (body if len(str(body)) < 80 else "...", text)
        # the item that is too long is named
        code, text = await status(input=[TOKENS, [7] * 513, TOKENS])
        assert code == 400 and "input 1" in text and "513" in text
        code, _ = await status(input=[TOKENS], encoding_format="hex")
        assert code in (400, 422)
        r = await client.post("/v1/embeddings",
                              json={"model": "nope", "input": "hi"})
        assert r.status_code == 404
        # the cap itself is accepted (checked without running 2048 items)
        from arks_amd.server.api import _embedding_items

        assert len(_embedding_items(["a"] * MAX_EMBEDDING_INPUTS,
                                    app.state.tokenizer)) == MAX_EMBEDDING_INPUTS

    run_with_client(app, fn)


def test_adapter_name_gives_another_vector(app):
    async def fn(client):
        out = {}
        for model in ("tiny", "a", "b"):
            r = await client.post("/v1/embeddings",
                                  json={"model": model, "input": [TOKENS]})
            assert r.status_code == 200, r.text
            assert r.json()["model"] == model
            out[model] = vec(r.json()["data"][0])
        assert np.abs(out["a"] - out["tiny"]).max() > 1e-3
        assert np.abs(out["a"] - out["b"]).max() > 1e-3

    run_with_client(app, fn)


def test_metrics_count_embedding_requests(app):
    async def fn(client):
        await embed(client, input=[TOKENS, TOKENS[:3]])
        text = (await client.get("/metrics")).text

        def value(name):
            return sum(float(l.rsplit(" ", 1)[1]) for l in text.splitlines()
                       if l.startswith(name + "{"))

        assert value("vllm:prompt_tokens_total") == 9
        assert value("vllm:generation_tokens_total") == 0
        assert value("vllm:request_success_total") == 2
        assert value("vllm:request_prompt_tokens_count") == 2

    run_with_client(app, fn)


def test_decode_instance_answers_400(tmp_path):
    app = make_app(tmp_path, disagg="decode")

    async def fn(client):
        r = await client.post("/v1/embeddings",
                              json={"model": "tiny", "input": "hi"})
        assert r.status_code == 400 and "decode" in r.text

    run_with_client(app, fn)


def test_disconnect_aborts_outstanding_items(app):
    """Cancelling the gathering call (what a client disconnect does) aborts
    every item that has not finished."""
    engine = app.state.engine

    async def fn(client):
        task = asyncio.ensure_future(engine.embed(
            "embd-x", [[7] * 300, [8] * 300, [9] * 300],
            {"mode": "mean", "normalize": True, "dims": None}))
        await asyncio.sleep(0)  # submitted, nothing stepped yet
        assert len(engine.streams) == 3
        task.cancel()
        with pytest.raises(asyncio.CancelledError):
            await task
        assert not engine.streams
        # the server still answers afterwards
        await embed(client, input=[TOKENS])
        assert not engine.engine.has_work()
        assert not engine.engine.runner._pool_slots

    run_with_client(app, fn)


def test_server_flags_reach_engine_config():
    from arks_amd.server.__main__ import build_engine_config, parse_args

    cfg = build_engine_config(parse_args(["--model", "preset:tiny"]))
    assert cfg.pooling == "auto" and cfg.embedding_normalize == "auto"
    cfg = build_engine_config(parse_args(
        ["--model", "preset:tiny", "--pooling", "mean",
         "--embedding-normalize", "false"]))
    assert cfg.pooling == "mean" and cfg.embedding_normalize == "false"
    with pytest.raises(SystemExit):
        parse_args(["--model", "preset:tiny", "--pooling", "max"])


def test_embedding_checkpoint_refuses_generation(app):
    """A model without an lm_head answers 400 on the generation routes."""
    app.state.engine.engine.runner.model.has_lm_head = False

    async def fn(client):
        r = await client.post("/v1/completions", json={
            "model": "tiny", "prompt": "hi", "max_tokens": 2})
        assert r.status_code == 400 and "embedding" in r.text
        r = await client.post("/v1/chat/completions", json={
            "model": "tiny", "max_tokens": 2,
            "messages": [{"role": "user", "content": "hi"}]})
        assert r.status_code == 400 and "embedding" in r.text
        await embed(client, input="still served")

    run_with_client(app, fn)


# ------------------------------ gateway ------------------------------------
@pytest.fixture()
def stack(app):
    """The gateway in front of the engine server, a token with request and
    token limits and a quota (as in test_gateway.py)."""
    store = Store()
    op = Operator(store)
    for doc in [
        {"apiVersion": "arks.ai/v1", "kind": "ArksEndpoint",
         "metadata": {"name": "tiny", "namespace": "default"},
         "spec": {"defaultWeight": 1}},
        {"apiVersion": "arks.ai/v1", "kind": "ArksQuota",
         "metadata": {"name": "q1", "namespace": "default"},
         "spec": {"quotas": [{"type": "prompt", "value": 100000},
                             {"type": "response", "value": 12},
                             {"type": "total", "value": 20}]}},
        {"apiVersion": "arks.ai/v1", "kind": "ArksToken",
         "metadata": {"name": "alice", "namespace": "default"},
         "spec": {"token": "sk-alice", "qos": [{
             "arksEndpoint": {"name": "tiny"},
             "rateLimits": [{"type": "rpm", "value": 10},
                            {"type": "tpm", "value": 1000}],
             "quota": {"name": "q1"}}]}},
    ]:
        store.create(parse_manifest(doc))
    op.reconcile_until_stable()
    route = store.get("HTTPRoute", "default", "tiny")
    route["spec"]["rules"][0]["backendRefs"] = [
        {"name": "arks-application-app1", "port": 8080, "weight": 1}]
    store.update(route)
    from arks_amd.gateway import RateLimiter

    gw = create_gateway_app(
        store, limiter=RateLimiter(clock=lambda: 1000.0),  # one fixed window
        transport=httpx.ASGITransport(app=app))
    return app, gw


def test_gateway_forwards_embeddings_and_accounts_prompt_tokens(stack):
    server_app, gw = stack

    async def go():
        async with server_app.router.lifespan_context(server_app):
            async with httpx.AsyncClient(
                transport=httpx.ASGITransport(app=gw), base_url="http://gw",
                timeout=60,
            ) as client:
                body = {"model": "tiny", "input": [TOKENS, TOKENS[:4]]}
                r = await client.post("/v1/embeddings", json=body)
                assert r.status_code == 401
                auth = {"Authorization": "Bearer sk-alice"}
                r = await client.post("/v1/embeddings", json=body,
                                      headers=auth)
                assert r.status_code == 200, r.text
                out = r.json()
                assert len(out["data"]) == 2
                assert out["usage"] == {"prompt_tokens": 10,
                                        "total_tokens": 10}
                qs = gw.state.quota_service
                assert qs.get_usage("default", "q1", "prompt") == 10
                assert qs.get_usage("default", "q1", "response") == 0
                assert qs.get_usage("default", "q1", "total") == 10
                # the token-type limit advanced by prompt_tokens, the
                # request-type limit by one
                counters = gw.state.limiter.store._data
                used = {rule: sum(v for k, (v, _) in counters.items()
                                  if f":{rule}:" in k)
                        for rule in ("tpm", "rpm")}
                assert used == {"tpm": 10, "rpm": 1}
                # a second and a third request: 20 then 30 > the quota of 20
                r = await client.post("/v1/embeddings", json=body,
                                      headers=auth)
                assert r.status_code == 200
                r = await client.post("/v1/embeddings", json=body,
                                      headers=auth)
                assert r.status_code == 200  # over only when current > limit
                r = await client.post("/v1/embeddings", json=body,
                                      headers=auth)
                assert r.status_code == 429 and "quota" in r.text
                assert qs.get_usage("default", "q1", "total") == 30

    asyncio.new_event_loop().run_until_complete(go())
