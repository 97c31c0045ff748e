"""Token table, token-level mask index and per-sequence matcher."""

from __future__ import annotations

import json
import threading
from collections import OrderedDict

import numpy as np

from .json_schema import any_object, choice_to_regex, schema_to_regex
from .regex_dfa import DFA, compile_regex

KINDS = ("json_schema", "json_object", "regex", "choice")


# ---------------------------------------------------------------- tokens ---
def _gpt2_unicode_to_byte() -> dict[str, int]:
    """Inverse of the GPT-2 byte<->unicode table used by byte-level BPE."""
    bs = (list(range(ord("!"), ord("~") + 1)) + list(range(0xA1, 0xAD))
          + list(range(0xAE, 0x100)))
    cs = bs[:]
    n = 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return {chr(c): b for b, c in zip(bs, cs)}


def token_bytes(tokenizer) -> list[bytes | None]:
    """The byte string each vocabulary id stands for, None for ids a grammar
    may never produce (special/added tokens, unused ids)."""
    offset = getattr(tokenizer, "OFFSET", None)
    if offset is not None and hasattr(tokenizer, "vocab_size") \
            and not hasattr(tokenizer, "tok"):
        return [bytes([i - offset]) if offset <= i < offset + 256 else None
                for i in range(tokenizer.vocab_size)]
    tok = getattr(tokenizer, "tok", tokenizer)
    vocab: dict[str, int] = tok.get_vocab()
    size = max(vocab.values()) + 1 if vocab else 0
    special = set(getattr(tok, "all_special_ids", ()) or ())
    added = getattr(tok, "get_added_vocab", None)
    if added is not None:
        special |= set(added().values())
    u2b = _gpt2_unicode_to_byte()
    # byte-level BPE writes a space as U+0120; sentencepiece as U+2581
    byte_level = any("Ġ" in p for p in vocab) and not any(
        "▁" in p for p in vocab)
    table: list[bytes | None] = [None] * size
    for piece, i in vocab.items():
        if i in special:
            continue
        if byte_level:
            try:
                table[i] = bytes(u2b[c] for c in piece)
            except KeyError:
                table[i] = None  # not a byte-level piece
        elif len(piece) == 6 and piece.startswith("<0x") and piece.endswith(">"):
            try:
                table[i] = bytes([int(piece[3:5], 16)])
            except ValueError:
                table[i] = piece.encode("utf-8")
        else:
            table[i] = piece.replace("▁", " ").encode("utf-8")
    return [t if t else None for t in table]


class TokenTable:
    """Trie over the token byte strings, built once per tokenizer."""

    def __init__(self, table: list[bytes | None], vocab_size: int,
                 eos_token_id: int):
        if len(table) > vocab_size:
            table = table[:vocab_size]
        self.vocab_size = vocab_size
        self.words = (vocab_size + 31) // 32
        self.eos_token_id = eos_token_id
        self.table = list(table) + [None] * (vocab_size - len(table))
        self.children: list[dict[int, int]] = [{}]
        self.tokens: list[list[int]] = [[]]
        for tid, bs in enumerate(self.table):
            if not bs or tid == eos_token_id:
                continue
            node = 0
            for b in bs:
                nxt = self.children[node].get(b)
                if nxt is None:
                    nxt = len(self.children)
                    self.children[node][b] = nxt
                    self.children.append({})
                    self.tokens.append([])
                node = nxt
            self.tokens[node].append(tid)

    @classmethod
    def from_tokenizer(cls, tokenizer, vocab_size: int, eos_token_id: int):
        return cls(token_bytes(tokenizer), vocab_size, eos_token_id)


# --------------------------------------------------------------- grammar ---
def canonical_spec(structured: dict) -> tuple[str, str]:
    """(kind, canonical text) of a SamplingParams.structured dict."""
    if not isinstance(structured, dict) or "kind" not in structured:
        raise ValueError("structured must be {'kind': ..., 'value': ...}")
    kind, value = structured["kind"], structured.get("value")
    if kind not in KINDS:
        raise ValueError(f"unknown structured kind {kind!r}: expected one of "
                         + ", ".join(KINDS))
    if kind == "json_schema" and isinstance(value, str):
        try:
            value = json.loads(value)
        except ValueError as e:
            raise ValueError(f"schema is not valid JSON: {e}") from None
    if kind == "choice" and isinstance(value, tuple):
        value = list(value)
    try:
        return kind, json.dumps(value, sort_keys=False, separators=(",", ":"))
    except TypeError as e:
        raise ValueError(f"structured value is not plain data: {e}") from None


def spec_to_regex(kind: str, canonical: str) -> str:
    value = json.loads(canonical)
    if kind == "regex":
        if not isinstance(value, str):
            raise ValueError("regex must be a string")
        return value
    if kind == "choice":
        return choice_to_regex(value)
    if kind == "json_object":
        return any_object()
    return schema_to_regex(value)


class CompiledGrammar:
    """A DFA bound to a token table: per DFA state, the allowed-token bitmask
    and the successor state of each allowed token, computed lazily by walking
    the token trie and the DFA together (cost ~ the trie nodes the state can
    reach, never a loop over the vocabulary)."""

    _next_uid = 0

    def __init__(self, dfa: DFA, tokens: TokenTable,
                 banned: tuple[int, ...] = ()):
        self.dfa = dfa
        self.tokens = tokens
        self.banned = tuple(sorted(set(banned)))
        self.eos_token_id = tokens.eos_token_id
        self._cache: dict[int, tuple[np.ndarray, dict[int, int]]] = {}
        CompiledGrammar._next_uid += 1
        self.uid = CompiledGrammar._next_uid

    def state(self, s: int) -> tuple[np.ndarray, dict[int, int]]:
        hit = self._cache.get(s)
        if hit is not None:
            return hit
        tt = self.tokens
        trans = self.dfa.trans
        succ: dict[int, int] = {}
        stack = [(0, s)]
        while stack:
            node, d = stack.pop()
            for tid in tt.tokens[node]:
                succ[tid] = d
            row = trans[d]
            for b, child in tt.children[node].items():
                nd = row.get(b)
                if nd is not None:
                    stack.append((child, nd))
        for tid in self.banned:
            succ.pop(tid, None)
        mask = np.zeros(tt.words, dtype=np.uint32)
        if succ:
            ids = np.fromiter(succ.keys(), dtype=np.int64, count=len(succ))
            np.bitwise_or.at(mask, ids >> 5,
                             (np.uint32(1) << (ids & 31).astype(np.uint32)))
        eos = self.eos_token_id
        if self.dfa.accepting[s] and 0 <= eos < tt.vocab_size:
            mask[eos >> 5] |= np.uint32(1) << np.uint32(eos & 31)
        mask.setflags(write=False)
        self._cache[s] = (mask, succ)
        return mask, succ


class GrammarMatcher:
    """Where one sequence stands in its grammar; a pure function of the
    tokens it was advanced by."""

    def __init__(self, compiled: CompiledGrammar):
        self.compiled = compiled
        self.state = 0
        self.is_terminated = False

    @property
    def key(self) -> tuple[int, int]:
        return self.compiled.uid, self.state

    def mask(self) -> np.ndarray:
        return self.compiled.state(self.state)[0]

    def advance(self, token_id: int) -> None:
        if self.is_terminated:
            raise ValueError("grammar already terminated")
        c = self.compiled
        if token_id == c.eos_token_id:
            # masked in every non-accepting state; it still arrives when a
            # state has no allowed token left (all of them in the request's
            # stop_token_ids) and the sampler ends the sequence
            self.is_terminated = True
            return
        nxt = c.state(self.state)[1].get(token_id)
        if nxt is None:
            raise ValueError(
                f"token {token_id} is not allowed by the grammar here")
        self.state = nxt


class GrammarCache:
    """LRU of compiled grammars keyed by (kind, canonical spec, banned)."""

    def __init__(self, tokens: TokenTable, max_states: int = 20000,
                 capacity: int = 64, lock=None):
        # lookups and inserts hold the lock; compiling runs outside it so
        # one slow grammar never blocks a request whose grammar is cached
        self._lock = lock if lock is not None else threading.Lock()
        self.tokens = tokens
        self.max_states = max_states
        self.capacity = capacity
        self._lru: OrderedDict = OrderedDict()
        self.compiles = 0

    def get(self, structured: dict,
            banned: tuple[int, ...] = ()) -> CompiledGrammar:
        kind, canon = canonical_spec(structured)
        key = (kind, canon, tuple(sorted(set(banned))))
        dfa = None
        with self._lock:
            hit = self._lru.get(key)
            if hit is not None:
                self._lru.move_to_end(key)
                return hit
            for (k2, c2, _), g in self._lru.items():  # same language
                if (k2, c2) == (kind, canon):
                    dfa = g.dfa
                    break
        if dfa is None:
            dfa = compile_regex(spec_to_regex(kind, canon), self.max_states)
            self.compiles += 1
            if not any(dfa.accepting):
                raise ValueError("the grammar matches no string at all")
        with self._lock:
            g = self._lru.get(key)  # another thread may have won the race
            if g is None:
                g = self._lru[key] = CompiledGrammar(dfa, self.tokens, key[2])
                while len(self._lru) > self.capacity:
                    self._lru.popitem(last=False)
        return g
