"""JSON Schema -> regex (the dialect of regex_dfa) for compact JSON.

The generated language has no insignificant whitespace: `{"a":1,"b":[2]}`.
Object properties come in declaration order; names absent from `required`
are optional; additional properties are never produced.
"""

from __future__ import annotations

import json

from .regex_dfa import escape_literal

STRING_CHAR = r'(?:[^"\\\x00-\x1f]|\\["\\/bfnrt]|\\u[0-9a-fA-F]{4})'
STRING = '"' + STRING_CHAR + '*"'
INTEGER = r"-?(?:0|[1-9][0-9]*)"
NUMBER = INTEGER + r"(?:\.[0-9]+)?(?:[eE][+-]?[0-9]+)?"
BOOLEAN = r"(?:true|false)"
NULL = r"null"

# json_object mode and untyped values: containers nest at most this deep
# (the top-level object counts as depth 1). A DFA cannot count unbounded
# nesting; deeper documents need a pushdown automaton, which is out of scope.
JSON_OBJECT_MAX_DEPTH = 5

_ANNOTATIONS = {"title", "description", "default", "examples", "$schema",
                "$id", "$comment", "$defs", "definitions"}
_KNOWN = _ANNOTATIONS | {
    "type", "enum", "const", "anyOf", "oneOf", "minLength", "maxLength",
    "pattern", "items", "minItems", "maxItems", "properties", "required",
    "additionalProperties", "$ref",
}


def _alt(parts: list[str]) -> str:
    return parts[0] if len(parts) == 1 else "(?:" + "|".join(parts) + ")"


def _dumps(value) -> str:
    return json.dumps(value, separators=(",", ":"), ensure_ascii=False)


def any_value(depth: int) -> str:
    """Any JSON value whose containers nest at most `depth` deep."""
    parts = [STRING, NUMBER, BOOLEAN, NULL]
    if depth > 0:
        parts += [any_array(depth), any_object(depth)]
    return _alt(parts)


def any_array(depth: int) -> str:
    v = any_value(depth - 1)
    return r"\[(?:" + v + "(?:," + v + r")*)?\]"


def any_object(depth: int = JSON_OBJECT_MAX_DEPTH) -> str:
    kv = STRING + ":" + any_value(depth - 1)
    return r"\{(?:" + kv + "(?:," + kv + r")*)?\}"


def _count(schema: dict, key: str, default):
    v = schema.get(key, default)
    if v is not None and (not isinstance(v, int) or isinstance(v, bool) or v < 0):
        raise ValueError(f"{key} must be a non-negative integer, got {v!r}")
    return v


class _Compiler:
    def __init__(self, root: dict):
        self.root = root
        self.ref_stack: list[str] = []

    def resolve(self, ref: str) -> dict:
        if not isinstance(ref, str) or not ref.startswith("#/"):
            raise ValueError(f"unsupported $ref {ref!r}: only local "
                             "'#/$defs/...' references are supported")
        node = self.root
        for part in ref[2:].split("/"):
            part = part.replace("~1", "/").replace("~0", "~")
            if not isinstance(node, dict) or part not in node:
                raise ValueError(f"unresolvable $ref {ref!r}")
            node = node[part]
        return node

    def compile(self, schema) -> str:
        if schema is True or schema == {}:
            return any_value(JSON_OBJECT_MAX_DEPTH - 1)
        if not isinstance(schema, dict):
            raise ValueError(f"schema must be an object, got {schema!r}")
        for key in schema:
            if key not in _KNOWN:
                raise ValueError(f"unsupported JSON Schema keyword {key!r}")
        if "$ref" in schema:
            ref = schema["$ref"]
            if ref in self.ref_stack:
                raise ValueError(f"recursive $ref {ref!r} is not supported")
            self.ref_stack.append(ref)
            try:
                return self.compile(self.resolve(ref))
            finally:
                self.ref_stack.pop()
        if "const" in schema:
            return escape_literal(_dumps(schema["const"]))
        if "enum" in schema:
            if not isinstance(schema["enum"], list) or not schema["enum"]:
                raise ValueError("enum must be a non-empty list")
            return _alt([escape_literal(_dumps(v)) for v in schema["enum"]])
        for key in ("anyOf", "oneOf"):
            if key in schema:
                if not isinstance(schema[key], list) or not schema[key]:
                    raise ValueError(f"{key} must be a non-empty list")
                return _alt([self.compile(s) for s in schema[key]])
        t = schema.get("type")
        if t is None:
            if "properties" in schema:
                t = "object"
            elif "items" in schema:
                t = "array"
            elif "pattern" in schema or "minLength" in schema or "maxLength" in schema:
                t = "string"
            else:
                return any_value(JSON_OBJECT_MAX_DEPTH - 1)
        if isinstance(t, list):
            if not t:
                raise ValueError("type list must not be empty")
            return _alt([self.typed(x, schema) for x in t])
        return self.typed(t, schema)

    def typed(self, t, schema: dict) -> str:
        if t == "string":
            return self.string(schema)
        if t == "integer":
            return INTEGER
        if t == "number":
            return NUMBER
        if t == "boolean":
            return BOOLEAN
        if t == "null":
            return NULL
        if t == "array":
            return self.array(schema)
        if t == "object":
            return self.object(schema)
        raise ValueError(f"unsupported type {t!r}")

    def string(self, schema: dict) -> str:
        if "pattern" in schema:
            if "minLength" in schema or "maxLength" in schema:
                raise ValueError("pattern together with minLength/maxLength "
                                 "is not supported")
            p = schema["pattern"]
            if not isinstance(p, str):
                raise ValueError("pattern must be a string")
            if p.startswith("^"):
                p = p[1:]
            if p.endswith("$") and not p.endswith("\\$"):
                p = p[:-1]
            return '"(?:' + p + ')"'
        lo = _count(schema, "minLength", 0)
        hi = _count(schema, "maxLength", None)
        if hi is None:
            rep = "*" if lo == 0 else "{%d,}" % lo
        else:
            if hi < lo:
                raise ValueError("maxLength is smaller than minLength")
            rep = "{%d,%d}" % (lo, hi)
        return '"' + STRING_CHAR + rep + '"'

    def array(self, schema: dict) -> str:
        items = schema.get("items", True)
        if isinstance(items, list):
            raise ValueError("unsupported JSON Schema keyword 'items' as a "
                             "list (tuple validation)")
        item = self.compile(items)
        lo = _count(schema, "minItems", 0)
        hi = _count(schema, "maxItems", None)
        if hi is not None and hi < lo:
            raise ValueError("maxItems is smaller than minItems")
        if hi == 0:
            return r"\[\]"
        more_lo = max(lo - 1, 0)
        more = ("{%d,}" % more_lo if more_lo else "*") if hi is None \
            else "{%d,%d}" % (more_lo, hi - 1)
        body = item + "(?:," + item + ")" + more
        return r"\[" + (body if lo >= 1 else "(?:" + body + ")?") + r"\]"

    def object(self, schema: dict) -> str:
        if "properties" not in schema:
            return any_object(JSON_OBJECT_MAX_DEPTH)
        props = schema["properties"]
        if not isinstance(props, dict):
            raise ValueError("properties must be an object")
        required = schema.get("required", [])
        for name in required:
            if name not in props:
                raise ValueError(f"required property {name!r} is not declared "
                                 "in properties")
        kvs = [(escape_literal(_dumps(k)) + ":" + self.compile(v), k in required)
               for k, v in props.items()]
        n = len(kvs)
        # after[i]: properties i.. when one was already written (comma first)
        after = [""] * (n + 1)
        for i in range(n - 1, -1, -1):
            kv, req = kvs[i]
            after[i] = ("," + kv if req else "(?:," + kv + ")?") + after[i + 1]
        # first[i]: properties i.. when none was written yet
        first = ""
        for i in range(n - 1, -1, -1):
            kv, req = kvs[i]
            here = kv + after[i + 1]
            first = here if req else "(?:" + here + "|" + first + ")"
        return r"\{" + first + r"\}"


def schema_to_regex(schema) -> str:
    if isinstance(schema, str):
        try:
            schema = json.loads(schema)
        except ValueError as e:
            raise ValueError(f"schema is not valid JSON: {e}") from None
    if not isinstance(schema, (dict, bool)):
        raise ValueError("schema must be a JSON object")
    return _Compiler(schema if isinstance(schema, dict) else {}).compile(schema)


def choice_to_regex(choices) -> str:
    if (not isinstance(choices, (list, tuple)) or not choices
            or not all(isinstance(c, str) and c for c in choices)):
        raise ValueError("choice must be a non-empty list of non-empty strings")
    return _alt([escape_literal(c) for c in choices])
