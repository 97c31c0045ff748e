"""Shared pieces of the structured-output engine tests: finite grammars (a
random-weight model must not be able to loop), their validators, and the
longest sentence of each, from which the tests derive max_tokens."""

import json
import re

from arks_amd.server.tokenizer import ByteTokenizer
from arks_amd.structured import compile_regex, spec_to_regex, canonical_spec

SCHEMA = {
    "type": "object",
    "properties": {
        "ok": {"type": "boolean"},
        "color": {"enum": ["red", "green", "blue"]},
        "code": {"type": "string", "pattern": "[A-Z]{3}"},
        "tags": {"type": "array", "items": {"enum": ["a", "b", "c"]},
                 "maxItems": 3},
    },
    "required": ["ok", "code"],
}
REGEX = r"(id|no)-[0-9]{2}(\.[a-f]{1,3})?"
CHOICES = ["yes", "no", "maybe", "日本"]

SPECS = {
    "json_schema": {"kind": "json_schema", "value": SCHEMA},
    "regex": {"kind": "regex", "value": REGEX},
    "choice": {"kind": "choice", "value": CHOICES},
}


def longest(spec: dict) -> int:
    """Bytes (= ByteTokenizer tokens) of the longest sentence; the grammar
    must be finite."""
    n = compile_regex(spec_to_regex(*canonical_spec(spec))).longest()
    assert n is not None, "test grammars must be finite languages"
    return n


# one more than the longest sentence leaves room for EOS; the tests assert
# this so truncation can never hide a failure
MAX_TOKENS = 80
for _s in SPECS.values():
    assert MAX_TOKENS >= longest(_s) + 1


def check_schema_doc(text: str) -> None:
    doc = json.loads(text)
    assert isinstance(doc, dict), text
    assert list(doc) == [k for k in SCHEMA["properties"] if k in doc], text
    assert set(doc) >= set(SCHEMA["required"]), text
    assert isinstance(doc["ok"], bool), text
    assert re.fullmatch("[A-Z]{3}", doc["code"]), text
    if "color" in doc:
        assert doc["color"] in ("red", "green", "blue"), text
    if "tags" in doc:
        assert isinstance(doc["tags"], list) and len(doc["tags"]) <= 3, text
        assert all(t in ("a", "b", "c") for t in doc["tags"]), text
    assert " " not in text and "\n" not in text, text


def check(kind: str, text: str) -> None:
    if kind == "json_schema":
        check_schema_doc(text)
    elif kind == "regex":
        assert re.fullmatch(REGEX, text), text
    else:
        assert text in CHOICES, text


def decode(token_ids: list[int], eos: int) -> str:
    """Output tokens -> text; the sentence must end in exactly one EOS."""
    assert token_ids and token_ids[-1] == eos, token_ids
    body = token_ids[:-1]
    assert eos not in body
    off = ByteTokenizer.OFFSET
    assert all(off <= t < off + 256 for t in body), body
    return bytes(t - off for t in body).decode("utf-8")
