"""Structured outputs over HTTP (CPU, preset tiny, ByteTokenizer):
response_format in its three forms, the guided_* extensions, 400s,
streaming and n > 1."""

import asyncio
import json

import httpx
import pytest

from arks_amd.config import EngineConfig
from arks_amd.server.api import create_app
from arks_amd.server.async_engine import AsyncEngine
from arks_amd.server.tokenizer import ByteTokenizer

from structured_testutil import (CHOICES, MAX_TOKENS, REGEX, SCHEMA, SPECS,
                                 check, longest)

MSGS = [{"role": "user", "content": "describe it"}]


@pytest.fixture()
def app():
    cfg = EngineConfig(preset="tiny", device="cpu", kv_cache_blocks=256,
                       max_model_len=512)
    engine = AsyncEngine(cfg, model_name="tiny")
    tok = ByteTokenizer(cfg.model_config().vocab_size, cfg.model_config().eos_token_id)
    return create_app(engine, "tiny", tok)


def run_with_client(app, fn):
    async def go():
        async with app.router.lifespan_context(app):
            transport = httpx.ASGITransport(app=app)
            async with httpx.AsyncClient(transport=transport, base_url="http://t",
                                         timeout=60) as client:
                await fn(client)

    asyncio.new_event_loop().run_until_complete(go())


def chat(**kw):
    for s in SPECS.values():
        assert MAX_TOKENS >= longest(s) + 1  # condition of the test
    return {"model": "tiny", "messages": MSGS, "max_tokens": MAX_TOKENS,
            "temperature": 0, **kw}


def test_response_format_three_forms(app):
    async def fn(client):
        r = await client.post("/v1/chat/completions", json=chat(
            response_format={"type": "json_schema", "json_schema": {
                "name": "thing", "schema": SCHEMA, "strict": True}}))
        assert r.status_code == 200, r.text
        c = r.json()["choices"][0]
        assert c["finish_reason"] == "stop"
        check("json_schema", c["message"]["content"])
        usage = r.json()["usage"]
        assert usage["completion_tokens"] == len(c["message"]["content"].encode()) + 1

        r = await client.post("/v1/chat/completions", json=chat(
            response_format={"type": "json_object"}, max_tokens=40,
            temperature=1.0, seed=0))
        assert r.status_code == 200, r.text
        c = r.json()["choices"][0]
        text = c["message"]["content"]
        if c["finish_reason"] == "stop":  # json_object is not a finite language
            assert isinstance(json.loads(text), dict)
        assert text.startswith("{")

        base = await client.post("/v1/chat/completions", json=chat(max_tokens=8))
        r = await client.post("/v1/chat/completions", json=chat(
            max_tokens=8, response_format={"type": "text"}))
        assert r.status_code == 200
        assert r.json()["choices"][0]["message"] == base.json()["choices"][0]["message"]

    run_with_client(app, fn)


def test_guided_extensions_chat_and_completions(app):
    async def fn(client):
        for body, kind in [
            ({"guided_json": SCHEMA}, "json_schema"),
            ({"guided_json": json.dumps(SCHEMA)}, "json_schema"),
            ({"guided_regex": REGEX}, "regex"),
            ({"guided_choice": CHOICES}, "choice"),
        ]:
            r = await client.post("/v1/chat/completions", json=chat(**body))
            assert r.status_code == 200, r.text
            c = r.json()["choices"][0]
            assert c["finish_reason"] == "stop"
            check(kind, c["message"]["content"])
            r = await client.post("/v1/completions", json={
                "model": "tiny", "prompt": "go:", "max_tokens": MAX_TOKENS,
                "temperature": 1.0, "seed": 5, **body})
            assert r.status_code == 200, r.text
            c = r.json()["choices"][0]
            assert c["finish_reason"] == "stop"
            check(kind, c["text"])

    run_with_client(app, fn)


def test_bad_requests_are_400(app):
    async def fn(client):
        recursive = {"$defs": {"n": {"type": "object", "properties": {
            "next": {"$ref": "#/$defs/n"}}}}, "$ref": "#/$defs/n"}
        for body, what in [
            ({"guided_regex": "a", "guided_choice": ["a"]}, "at most one"),
            ({"response_format": {"type": "json_object"}, "guided_json": {}},
             "at most one"),
            ({"guided_json": recursive}, "recursive"),
            ({"response_format": {"type": "json_schema",
                                  "json_schema": {"name": "r", "schema": recursive}}},
             "recursive"),
            ({"guided_regex": "(?=a)b"}, "lookaround"),
            ({"guided_regex": "a", "ignore_eos": True}, "ignore_eos"),
            ({"response_format": {"type": "json_schema"}}, "schema is required"),
        ]:
            r = await client.post("/v1/chat/completions", json=chat(**body))
            assert r.status_code == 400, (body, r.text)
            assert what in r.json()["error"]["message"], r.text
        r = await client.post("/v1/completions", json={
            "model": "tiny", "prompt": "x", "guided_regex": r"(a)\1"})
        assert r.status_code == 400
        assert "backreference" in r.json()["error"]["message"]
        # the engine still serves
        r = await client.post("/v1/chat/completions", json=chat(guided_choice=CHOICES))
        assert r.status_code == 200

    run_with_client(app, fn)


def test_streaming(app):
    async def fn(client):
        text, finish = "", None
        async with client.stream("POST", "/v1/chat/completions", json=chat(
                guided_json=SCHEMA, stream=True, temperature=1.0, seed=11)) as r:
            assert r.status_code == 200
            async for line in r.aiter_lines():
                if not line.startswith("data: ") or line == "data: [DONE]":
                    continue
                for c in json.loads(line[6:])["choices"]:
                    text += c["delta"].get("content") or ""
                    finish = c.get("finish_reason") or finish
        assert finish == "stop"
        check("json_schema", text)

    run_with_client(app, fn)


def test_n2(app):
    async def fn(client):
        r = await client.post("/v1/chat/completions", json=chat(
            guided_json=SCHEMA, n=2, temperature=1.0, seed=3))
        assert r.status_code == 200, r.text
        choices = r.json()["choices"]
        assert len(choices) == 2
        for c in choices:
            assert c["finish_reason"] == "stop"
            check("json_schema", c["message"]["content"])

    run_with_client(app, fn)


def test_fields_are_in_the_openapi_schema(app):
    props = app.openapi()["components"]["schemas"]
    chat_props = props["ChatCompletionRequest"]["properties"]
    for f in ("response_format", "guided_json", "guided_regex", "guided_choice"):
        assert f in chat_props
    for f in ("guided_json", "guided_regex", "guided_choice"):
        assert f in props["CompletionRequest"]["properties"]
