"""Structured outputs, CPU: regex -> DFA against `re`, rejections, JSON
Schema -> regex, the token index against a brute-force walk, token tables,
and the plain-torch masked sampling ops."""

import json
import random
import re

import numpy as np
import pytest
import torch
from hypothesis import given, settings
from hypothesis import strategies as st

from arks_amd.ops import ref
from arks_amd.server.tokenizer import ByteTokenizer
from arks_amd.structured import (CompiledGrammar, GrammarCache,
                                 GrammarMatcher, TokenTable, choice_to_regex,
                                 compile_regex, schema_to_regex, token_bytes)

# together: literals, '.', every escape, classes, negated classes, groups,
# non-capturing groups, alternation, ? * + {m} {m,} {m,n}, anchors,
# non-ASCII literals and '.'/negated classes over multi-byte input
PATTERNS = [
    r"abc",
    r"a.c",
    r".*",
    r".+x",
    r"\d+",
    r"\w*\s\w+",
    r"\D\d",
    r"\W+",
    r"\S{2}",
    r"a\n\t\r\\b",
    r"\.\*\+\?\(\)\[\]\{\}\|\^\$",
    r"\x41\x62",
    r"é+",
    r"[abc]+",
    r"[a-cx-z0-3]*",
    r"[^abc]",
    r"[^a-c\d]+",
    r"[\w.-]+@[\w-]+",
    r"[\]\-a]+",
    r"(ab|cd)*e",
    r"(?:a|bc|)d",
    r"a?b*c+",
    r"a{3}",
    r"a{2,}b",
    r"(?:ab){1,3}",
    r"^ab$",
    r"é|ü+|日本",
    r"x.y",
    r"[éa]b",
    r"(a|b)(c|d){0,2}[^é]",
]
ALPHABET = "abcdexyz019 .\n\t-@_AZé日ü\\()[]{}|^$*+?"


@pytest.fixture(scope="module")
def dfas():
    return {p: compile_regex(p) for p in PATTERNS}


def _agree(p, dfa, s):
    want = bool(re.fullmatch(p, s, re.ASCII))
    assert dfa.fullmatch(s.encode("utf-8")) == want, (p, s)


@settings(max_examples=150, deadline=None)
@given(st.text(alphabet=ALPHABET, max_size=8))
def test_dfa_matches_re_on_random_text(dfas, s):
    for p, dfa in dfas.items():
        _agree(p, dfa, s)


def _walks(dfa, rng, n=40, max_len=12):
    out = []
    for _ in range(n):
        s, bs = 0, bytearray()
        for _ in range(rng.randrange(max_len + 1)):
            if not dfa.trans[s]:
                break
            b = rng.choice(sorted(dfa.trans[s]))
            bs.append(b)
            s = dfa.trans[s][b]
        out.append(bytes(bs))
    return out


@pytest.mark.parametrize("p", PATTERNS)
def test_dfa_matches_re_on_walks_and_mutations(dfas, p):
    """Random walks of the DFA itself (mostly inside the language's
    prefixes) and one-byte mutations of them (mostly just outside)."""
    rng = random.Random(hash(p) & 0xFFFF)
    dfa = dfas[p]
    cases = _walks(dfa, rng)
    for w in list(cases):
        if w:
            i = rng.randrange(len(w))
            cases.append(w[:i] + bytes([rng.randrange(256)]) + w[i + 1:])
            cases.append(w[:i] + w[i + 1:])
    checked = 0
    for bs in cases:
        try:
            s = bs.decode("utf-8")
        except UnicodeDecodeError:
            # not text: `re` cannot be asked; the DFA must refuse ill-formed
            # UTF-8 unless the pattern spells those bytes itself
            continue
        _agree(p, dfa, s)
        checked += 1
    assert checked >= 20


def test_dfa_rejects_ill_formed_utf8():
    dfa = compile_regex(r".+")
    for bad in (b"\xff", b"\xc0\x80", b"\xe0\x80\x80", b"\xed\xa0\x80",
                b"\xf4\x90\x80\x80", b"\xc3", b"a\x80"):
        assert not dfa.fullmatch(bad)
    assert dfa.fullmatch("é日😀".encode())


def test_dfa_is_trimmed():
    dfa = compile_regex(r"ab(c|d)e|abx{2}")
    # every state can reach an accepting state
    can = {s for s, a in enumerate(dfa.accepting) if a}
    changed = True
    while changed:
        changed = False
        for s, row in enumerate(dfa.trans):
            if s not in can and any(n in can for n in row.values()):
                can.add(s)
                changed = True
    assert can == set(range(dfa.num_states))


@pytest.mark.parametrize("p,what", [
    (r"(a)\1", "backreference"),
    (r"(?=a)a", "lookaround"),
    (r"(?!a)b", "lookaround"),
    (r"(?<=a)b", "lookaround"),
    (r"a*?", "lazy"),
    (r"a+?", "lazy"),
    (r"a{1,2}?", "lazy"),
    (r"a*+", "possessive"),
    (r"(?i)abc", "inline flags"),
    (r"[a-é]", "non-ASCII endpoint"),
    (r"\bword", "escape"),
])
def test_unsupported_constructs_are_named(p, what):
    with pytest.raises(ValueError, match=what):
        compile_regex(p)


def test_state_cap():
    with pytest.raises(ValueError, match="too large"):
        compile_regex(r"(a|b)*a(a|b){12}", max_states=500)
    assert compile_regex(r"(a|b)*a(a|b){3}", max_states=500).num_states <= 500


# ------------------------------------------------------------- schema ------
def _is_int(v):
    return isinstance(v, int) and not isinstance(v, bool)


SCHEMA_CASES = [
    # (schema, accepted documents, rejected documents, structural check)
    ({"type": "string"}, ['"a"', '""', '"é\\n\\u00e9"'], ['a', '"a', '"a"b"', '"\n"'],
     lambda v: isinstance(v, str)),
    ({"type": "string", "minLength": 2, "maxLength": 3}, ['"ab"', '"abc"'],
     ['"a"', '"abcd"'], lambda v: isinstance(v, str) and 2 <= len(v) <= 3),
    ({"type": "string", "pattern": "^[A-Z]{3}$"}, ['"ABC"'], ['"AB"', '"abc"', 'ABC'],
     lambda v: re.fullmatch("[A-Z]{3}", v) is not None),
    ({"type": "integer"}, ["0", "-12", "7"], ["01", "1.5", "+1", "--1", ""], _is_int),
    ({"type": "number"}, ["0", "-1.5", "2e10", "3.25E-2"], ["1.", ".5", "1e", "0x1"],
     lambda v: isinstance(v, (int, float)) and not isinstance(v, bool)),
    ({"type": "boolean"}, ["true", "false"], ["True", "1", "null"],
     lambda v: isinstance(v, bool)),
    ({"type": "null"}, ["null"], ["None", "0"], lambda v: v is None),
    ({"type": ["integer", "null"]}, ["3", "null"], ['"3"', "true"],
     lambda v: v is None or _is_int(v)),
    ({"enum": ["red", 3, None, "a|b"]}, ['"red"', "3", "null", '"a|b"'],
     ['"a"', '"blue"', "4"], lambda v: v in ("red", 3, None, "a|b")),
    ({"const": {"k": [1, "x"]}}, ['{"k":[1,"x"]}'], ['{"k": [1,"x"]}', '{}'],
     lambda v: v == {"k": [1, "x"]}),
    ({"anyOf": [{"type": "boolean"}, {"type": "integer"}]}, ["true", "5"], ['"x"'],
     lambda v: isinstance(v, bool) or _is_int(v)),
    ({"oneOf": [{"const": "a"}, {"type": "null"}]}, ['"a"', "null"], ['"b"'],
     lambda v: v in ("a", None)),
    ({"type": "array", "items": {"type": "integer"}}, ["[]", "[1]", "[1,2,3]"],
     ["[1,]", "[1, 2]", "[,1]", '["a"]', "["],
     lambda v: isinstance(v, list) and all(_is_int(x) for x in v)),
    ({"type": "array", "items": {"type": "boolean"}, "minItems": 1, "maxItems": 2},
     ["[true]", "[true,false]"], ["[]", "[true,true,true]"],
     lambda v: isinstance(v, list) and 1 <= len(v) <= 2),
    ({"type": "array", "items": {"type": "null"}, "minItems": 2},
     ["[null,null]", "[null,null,null]"], ["[null]", "[]"],
     lambda v: isinstance(v, list) and len(v) >= 2),
    ({"type": "object",
      "properties": {"a": {"type": "integer"}, "b": {"type": "boolean"},
                     "c": {"type": "null"}},
      "required": ["b"]},
     ['{"b":true}', '{"a":1,"b":false}', '{"b":true,"c":null}',
      '{"a":0,"b":true,"c":null}'],
     ['{}', '{"a":1}', '{"b":true,"a":1}', '{"b":true,}', '{"b":true,"d":1}',
      '{"b": true}', '{,"b":true}'],
     lambda v: isinstance(v, dict) and "b" in v and set(v) <= {"a", "b", "c"}),
    ({"type": "object", "properties": {"a": {"type": "integer"},
                                       "b": {"type": "integer"}}},
     ['{}', '{"a":1}', '{"b":2}', '{"a":1,"b":2}'], ['{"a":1,}', '{,"b":2}', '{"b":2,"a":1}'],
     lambda v: isinstance(v, dict) and set(v) <= {"a", "b"}),
    ({"$defs": {"pt": {"type": "object", "properties": {"x": {"type": "integer"}},
                       "required": ["x"]}},
      "type": "array", "items": {"$ref": "#/$defs/pt"}, "maxItems": 2},
     ['[]', '[{"x":1}]', '[{"x":1},{"x":-2}]'], ['[{}]', '[{"x":1},{"x":1},{"x":1}]'],
     lambda v: all(set(p) == {"x"} for p in v)),
    ({"definitions": {"b": {"type": "boolean"}}, "$ref": "#/definitions/b",
      "title": "t", "description": "d", "default": True, "examples": [False]},
     ["true"], ["1"], lambda v: isinstance(v, bool)),
]


@pytest.mark.parametrize("schema,accept,reject,check", SCHEMA_CASES)
def test_schema_to_regex(schema, accept, reject, check):
    rx = schema_to_regex(schema)
    dfa = compile_regex(rx)
    for doc in accept:
        assert dfa.fullmatch(doc.encode()), doc
        assert re.fullmatch(rx, doc, re.ASCII), doc
        assert check(json.loads(doc)), doc
    for doc in reject:
        assert not dfa.fullmatch(doc.encode()), doc


@pytest.mark.parametrize("schema,what", [
    ({"$defs": {"n": {"type": "object", "properties": {"next": {"$ref": "#/$defs/n"}}}},
      "$ref": "#/$defs/n"}, "recursive"),
    ({"not": {"type": "null"}}, "not"),
    ({"if": {}, "then": {}}, "if"),
    ({"type": "object", "patternProperties": {"a": {}}}, "patternProperties"),
    ({"type": "integer", "multipleOf": 2}, "multipleOf"),
    ({"type": "widget"}, "widget"),
    ({"$ref": "http://example.com/s.json"}, r"\$ref"),
])
def test_schema_rejections(schema, what):
    with pytest.raises(ValueError, match=what):
        schema_to_regex(schema)


def test_json_object_mode_depth_and_whitespace():
    from arks_amd.structured import JSON_OBJECT_MAX_DEPTH, any_object

    assert JSON_OBJECT_MAX_DEPTH == 5
    dfa = compile_regex(any_object())
    assert dfa.num_states <= 20000
    assert dfa.fullmatch(b'{}')
    assert dfa.fullmatch(b'{"a":[1,{"b":[{"c":null}]}],"d":"x y"}')  # depth 5
    assert not dfa.fullmatch(b'{"a":[1,{"b":[{"c":[]}]}]}')  # depth 6
    assert not dfa.fullmatch(b'{"a": 1}')
    assert not dfa.fullmatch(b'{"a":1} ')
    assert not dfa.fullmatch(b'[1]')


def test_choice():
    rx = choice_to_regex(["yes", "no?", "a|b", "日本"])
    dfa = compile_regex(rx)
    for c in ("yes", "no?", "a|b", "日本"):
        assert dfa.fullmatch(c.encode())
    for c in ("no", "a", "b", "yesno", ""):
        assert not dfa.fullmatch(c.encode())
    with pytest.raises(ValueError):
        choice_to_regex([])


# -------------------------------------------------------- token index ------
EOS = 2
SENTENCES = [
    '{"name":"Ada","tags":["x","y"],"ok":true}',
    '{"ok":false,"code":"XYZ"}',
    'yes no maybe 2024-01-31 12:30',
    '"quoted", text": more',
    'naïve café 日本語',
]


def _byte_table():
    return TokenTable.from_tokenizer(ByteTokenizer(512, EOS), 512, EOS)


def _synthetic_table():
    rng = random.Random(7)
    table = [None, None, None, None] + [bytes([b]) for b in range(256)]
    pieces = set()
    while len(pieces) < 300:
        s = rng.choice(SENTENCES).encode()
        i = rng.randrange(len(s) - 1)
        pieces.add(s[i:i + rng.randrange(2, 7)])
    # tokens that straddle a string delimiter
    pieces |= {b'":"', b'","', b'"],"', b'":', b'"}', b'a"', b'":["'}
    table += sorted(p for p in pieces if len(p) > 1)
    return TokenTable(table, len(table) + 5, EOS)  # a few unused ids on top


GRAMMARS = [
    schema_to_regex({"type": "object", "properties": {
        "name": {"type": "string", "maxLength": 4},
        "tags": {"type": "array", "items": {"enum": ["x", "y"]}, "maxItems": 2},
        "ok": {"type": "boolean"}}, "required": ["ok"]}),
    r"(yes|no|maybe) \d{4}-\d{2}-\d{2}",
    r'"[^"]*", .+',
]


@pytest.mark.parametrize("make_table", [_byte_table, _synthetic_table])
@pytest.mark.parametrize("rx", GRAMMARS)
def test_token_index_equals_brute_force(make_table, rx):
    tt = make_table()
    dfa = compile_regex(rx)
    g = CompiledGrammar(dfa, tt)
    for s in range(dfa.num_states):  # every state is reachable (trimmed)
        mask, succ = g.state(s)
        want = {}
        for tid, bs in enumerate(tt.table):
            if bs is None or tid == EOS:
                continue
            d = s
            for b in bs:
                d = dfa.trans[d].get(b, -1)
                if d < 0:
                    break
            if d >= 0:
                want[tid] = d
        assert succ == want
        bits = {t for t in range(tt.vocab_size) if (int(mask[t >> 5]) >> (t & 31)) & 1}
        assert bits - {EOS} == set(want)
        assert (EOS in bits) == dfa.accepting[s]
        if dfa.accepting[s] and not dfa.trans[s]:
            assert bits == {EOS}
        assert mask.dtype == np.uint32 and mask.shape == ((tt.vocab_size + 31) // 32,)


def test_banned_stop_tokens_are_never_allowed():
    tt = _byte_table()
    a = ByteTokenizer.OFFSET + ord("a")
    g = CompiledGrammar(compile_regex("a|b"), tt, banned=(a,))
    mask, succ = g.state(0)
    assert a not in succ and not (int(mask[a >> 5]) >> (a & 31)) & 1
    assert ByteTokenizer.OFFSET + ord("b") in succ


def test_matcher_and_cache():
    tt = _byte_table()
    cache = GrammarCache(tt)
    g = cache.get({"kind": "choice", "value": ["ab", "a"]})
    assert cache.get({"kind": "choice", "value": ["ab", "a"]}) is g
    assert cache.compiles == 1
    m = GrammarMatcher(g)
    off = ByteTokenizer.OFFSET
    assert not (int(m.mask()[EOS >> 5]) >> EOS) & 1
    m.advance(off + ord("a"))
    assert (int(m.mask()[EOS >> 5]) >> EOS) & 1  # "a" is a sentence
    with pytest.raises(ValueError):
        m.advance(off + ord("c"))
    m.advance(off + ord("b"))
    m.advance(EOS)
    assert m.is_terminated
    for bad in ({"kind": "regex", "value": "(?=a)"}, {"kind": "nope", "value": 1},
                {"kind": "json_schema", "value": {"not": {}}}, {"value": "a"}):
        with pytest.raises(ValueError):
            cache.get(bad)


# -------------------------------------------------------- token tables -----
class _FakeHF:
    """The slice of the HF tokenizer interface token_bytes reads."""

    def __init__(self, vocab, special):
        self._vocab, self._special = vocab, special
        self.all_special_ids = [vocab[s] for s in special]

    def get_vocab(self):
        return dict(self._vocab)

    def get_added_vocab(self):
        return {s: self._vocab[s] for s in self._special}


def test_token_bytes_byte_tokenizer():
    t = token_bytes(ByteTokenizer(512, 2))
    assert len(t) == 512
    assert t[:4] == [None] * 4 and t[4] == b"\x00" and t[259] == b"\xff"
    assert all(x is None for x in t[260:])


def test_token_bytes_byte_level_bpe():
    vocab = {"Ġhello": 0, "Ċ": 1, "a": 2, "Ã©": 3, "<|endoftext|>": 4, "ĠĠ": 6}
    t = token_bytes(_FakeHF(vocab, ["<|endoftext|>"]))
    assert t == [b" hello", b"\n", b"a", "é".encode(), None, None, b"  "]


def test_token_bytes_sentencepiece():
    vocab = {"<unk>": 0, "<s>": 1, "▁the": 2, "<0x0A>": 3, "é": 4, "▁": 5,
             "<0xZZ>": 6}
    t = token_bytes(_FakeHF(vocab, ["<unk>", "<s>"]))
    assert t == [None, None, b" the", b"\n", "é".encode(), b" ", b"<0xZZ>"]


# ------------------------------------------------------------ ref ops ------
def _pack(allowed: torch.Tensor) -> torch.Tensor:
    """[slots, V] bool -> [slots, ceil(V/32)] int32."""
    slots, v = allowed.shape
    words = (v + 31) // 32
    a = np.zeros((slots, words * 32), dtype=np.uint64)
    a[:, :v] = allowed.numpy()
    packed = (a.reshape(slots, words, 32) << np.arange(32, dtype=np.uint64)).sum(-1)
    return torch.from_numpy(packed.astype(np.uint32).view(np.int32).copy())


def test_ref_masked_ops_agree_with_where():
    g = torch.Generator().manual_seed(0)
    rows, v = 6, 77  # partial last word
    logits = torch.randn(rows, v, generator=g).bfloat16()
    allowed = torch.rand(3, v, generator=g) < 0.5
    masks = _pack(allowed)
    masks[:, -1] |= torch.tensor(-1 << (v % 32), dtype=torch.int32)  # junk bits >= V
    mask_row = torch.tensor([0, -1, 2, 1, 0, -1], dtype=torch.int32)
    full = torch.stack([allowed[r] if r >= 0 else torch.ones(v, dtype=torch.bool)
                        for r in mask_row.tolist()])
    masked = torch.where(full, logits.float(), float("-inf"))
    assert torch.equal(ref.greedy_sample_masked(logits, masks, mask_row),
                       ref.greedy_sample(masked))
    u = torch.rand(rows, v, generator=g)
    t = torch.tensor([0.0, 1.0, 0.7, 1.3, 0.0, 2.0])
    assert torch.equal(ref.gumbel_sample_masked(logits, t, u, masks, mask_row),
                       ref.gumbel_sample(masked, t, u))
    for dt in (torch.bfloat16, torch.float32):
        x = logits.to(dt).clone()
        ref.apply_token_bitmask(x, masks, mask_row)
        assert torch.equal(x, torch.where(full, logits.to(dt), float("-inf")))
    # an empty mask gives -1; a masked +inf / NaN never wins
    empty = torch.zeros(1, 3, dtype=torch.int32)
    assert ref.greedy_sample_masked(logits[:1], empty, torch.zeros(1, dtype=torch.int32)).tolist() == [-1]
    x = torch.zeros(2, v).bfloat16()
    x[0, 5] = float("inf")
    x[1, 5] = float("nan")
    only = torch.zeros(1, v, dtype=torch.bool)
    only[0, 9] = True
    assert ref.greedy_sample_masked(x, _pack(only), torch.zeros(2, dtype=torch.int32)).tolist() == [9, 9]
