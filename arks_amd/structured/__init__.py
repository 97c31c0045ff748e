"""Structured outputs: constrain generation to a regex, a JSON Schema, any
JSON object, or one of a list of choices.

A spec compiles to a byte-level DFA (regex_dfa, json_schema); a
CompiledGrammar binds it to the tokenizer's vocabulary and yields, per DFA
state, a packed allowed-token bitmask that the masked sampling kernels
(ops.greedy_sample_masked, ops.sample_tokens_masked, ops.apply_token_bitmask)
consume. See docs/engine.md, "Structured outputs".
"""

from .grammar import (CompiledGrammar, GrammarCache, GrammarMatcher,
                      TokenTable, canonical_spec, spec_to_regex, token_bytes)
from .json_schema import (JSON_OBJECT_MAX_DEPTH, any_object, choice_to_regex,
                          schema_to_regex)
from .regex_dfa import DFA, compile_regex, escape_literal

__all__ = [
    "CompiledGrammar", "DFA", "GrammarCache", "GrammarMatcher",
    "JSON_OBJECT_MAX_DEPTH", "TokenTable", "any_object", "canonical_spec",
    "choice_to_regex", "compile_regex", "escape_literal", "schema_to_regex",
    "spec_to_regex", "token_bytes",
]
