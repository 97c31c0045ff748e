"""Regex -> byte-level DFA with full-match semantics.

Pipeline: parse -> Thompson NFA over bytes -> subset construction -> trim
(every kept state is reachable and can still reach an accepting state).

The automaton runs over UTF-8 bytes: a non-ASCII literal is its encoding,
and `.`, negated classes and \\D \\W \\S match one well-formed code point.
Escapes \\d \\w \\s are ASCII (like `re.ASCII`); `.` excludes "\\n".
"""

from __future__ import annotations

_DIGIT = frozenset(range(0x30, 0x3A))
_WORD = frozenset(
    list(range(0x30, 0x3A)) + list(range(0x41, 0x5B))
    + list(range(0x61, 0x7B)) + [0x5F]
)
_SPACE = frozenset(b" \t\n\r\f\v")
_ASCII = frozenset(range(0x80))
_CONT = frozenset(range(0x80, 0xC0))
# well-formed multi-byte UTF-8 (RFC 3629, no surrogates, <= U+10FFFF)
_MULTI = (
    (range(0xC2, 0xE0), _CONT),
    (range(0xE0, 0xE1), range(0xA0, 0xC0), _CONT),
    (range(0xE1, 0xED), _CONT, _CONT),
    (range(0xED, 0xEE), range(0x80, 0xA0), _CONT),
    (range(0xEE, 0xF0), _CONT, _CONT),
    (range(0xF0, 0xF1), range(0x90, 0xC0), _CONT, _CONT),
    (range(0xF1, 0xF4), _CONT, _CONT, _CONT),
    (range(0xF4, 0xF5), range(0x80, 0x90), _CONT, _CONT),
)
_META = set("\\.[]()|?*+{}^$")
_MAX_REPEAT = 1000

# AST: ("set", frozenset[int]) one byte of the set; ("cat", [nodes]);
# ("alt", [nodes]); ("rep", node, lo, hi|None)


def _seq(parts) -> tuple:
    return ("cat", [("set", frozenset(p)) for p in parts])


def _codepoint(ascii_set: frozenset, multibyte: bool) -> tuple:
    alts = [("set", ascii_set)] if ascii_set else []
    if multibyte:
        alts += [_seq(p) for p in _MULTI]
    return ("alt", alts)


def _literal(ch: str) -> tuple:
    bs = ch.encode("utf-8")
    if len(bs) == 1:
        return ("set", frozenset(bs))
    return ("cat", [("set", frozenset([b])) for b in bs])


class _Parser:
    def __init__(self, pattern: str):
        self.p = pattern
        self.i = 0

    def error(self, what: str) -> ValueError:
        return ValueError(f"unsupported regex construct: {what} "
                          f"(at offset {self.i} of {self.p!r})")

    def peek(self) -> str:
        return self.p[self.i] if self.i < len(self.p) else ""

    def parse(self) -> tuple:
        if self.p.startswith("^"):
            self.i = 1
        node = self.alt()
        if self.i < len(self.p):
            raise ValueError(f"unbalanced ')' at offset {self.i} of {self.p!r}")
        return node

    def alt(self) -> tuple:
        branches = [self.cat()]
        while self.peek() == "|":
            self.i += 1
            branches.append(self.cat())
        return branches[0] if len(branches) == 1 else ("alt", branches)

    def cat(self) -> tuple:
        items = []
        while self.i < len(self.p) and self.peek() not in "|)":
            if self.peek() == "$" and (self.i == len(self.p) - 1):
                self.i += 1  # trailing anchor: full-match anyway
                break
            items.append(self.quantified())
        return ("cat", items)

    def quantified(self) -> tuple:
        node = self.atom()
        while True:
            c = self.peek()
            if c == "?":
                lo, hi = 0, 1
            elif c == "*":
                lo, hi = 0, None
            elif c == "+":
                lo, hi = 1, None
            elif c == "{":
                rng = self.braces()
                if rng is None:
                    return node
                lo, hi = rng
                self.i -= 1
            else:
                return node
            self.i += 1
            if self.peek() == "?":
                raise self.error("lazy quantifier")
            if self.peek() == "+":
                raise self.error("possessive quantifier")
            node = ("rep", node, lo, hi)

    def braces(self):
        """Parse {m} {m,} {m,n} at self.i; leaves self.i past the '}'."""
        j = self.p.find("}", self.i)
        body = self.p[self.i + 1:j] if j > 0 else ""
        parts = body.split(",")
        if j < 0 or len(parts) > 2 or not parts[0].isdigit() or (
                len(parts) == 2 and parts[1] and not parts[1].isdigit()):
            raise self.error("malformed {m,n} quantifier")
        lo = int(parts[0])
        hi = lo if len(parts) == 1 else (int(parts[1]) if parts[1] else None)
        if hi is not None and hi < lo or max(lo, hi or 0) > _MAX_REPEAT:
            raise self.error(f"repeat bounds {{{body}}}")
        self.i = j + 1
        return lo, hi

    def atom(self) -> tuple:
        c = self.peek()
        self.i += 1
        if c == "(":
            if self.peek() == "?":
                nxt = self.p[self.i + 1:self.i + 3]
                if nxt[:1] == ":":
                    self.i += 2
                elif nxt[:1] in ("=", "!") or nxt in ("<=", "<!"):
                    raise self.error("lookaround")
                elif nxt[:1] == "P" or nxt[:1] == "<":
                    raise self.error("named group")
                else:
                    raise self.error("inline flags")
            node = self.alt()
            if self.peek() != ")":
                raise ValueError(f"missing ')' in {self.p!r}")
            self.i += 1
            return node
        if c == "[":
            return self.char_class()
        if c == ".":
            return _codepoint(_ASCII - {0x0A}, True)
        if c == "\\":
            kind, val = self.escape()
            if kind == "set":
                return ("set", val)
            if kind == "neg":
                return _codepoint(_ASCII - val, True)
            return _literal(val)
        if c in "*+?{":
            raise self.error(f"nothing to repeat before {c!r}")
        if c in "^$":
            raise self.error(f"anchor {c!r} inside the pattern")
        return _literal(c)

    def escape(self):
        """After a backslash. ("set"|"neg", byteset) or ("chr", char)."""
        c = self.peek()
        if not c:
            raise self.error("trailing backslash")
        self.i += 1
        if c in "dws":
            return "set", {"d": _DIGIT, "w": _WORD, "s": _SPACE}[c]
        if c in "DWS":
            return "neg", {"D": _DIGIT, "W": _WORD, "S": _SPACE}[c]
        if c in "ntrfv0":
            return "chr", {"n": "\n", "t": "\t", "r": "\r", "f": "\f",
                           "v": "\v", "0": "\0"}[c]
        if c in "xu":
            n = 2 if c == "x" else 4
            h = self.p[self.i:self.i + n]
            if len(h) != n or any(ch not in "0123456789abcdefABCDEF" for ch in h):
                raise self.error(f"malformed \\{c} escape")
            self.i += n
            return "chr", chr(int(h, 16))
        if c.isdigit():
            raise self.error("backreference")
        if c in "bBAZzGkpPNU":
            raise self.error(f"escape \\{c}")
        if c.isalnum():
            raise self.error(f"unknown escape \\{c}")
        return "chr", c

    def char_class(self) -> tuple:
        negate = self.peek() == "^"
        if negate:
            self.i += 1
        ascii_set: set[int] = set()
        wide: list[str] = []  # non-ASCII single characters
        neg_escapes: list[frozenset] = []
        first = True
        while True:
            c = self.peek()
            if not c:
                raise ValueError(f"missing ']' in {self.p!r}")
            if c == "]" and not first:
                self.i += 1
                break
            first = False
            self.i += 1
            if c == "\\":
                kind, val = self.escape()
                if kind == "set":
                    ascii_set |= val
                    continue
                if kind == "neg":
                    neg_escapes.append(val)
                    continue
                c = val
            if self.peek() == "-" and self.p[self.i + 1:self.i + 2] not in ("]", ""):
                self.i += 1
                hi = self.peek()
                self.i += 1
                if hi == "\\":
                    kind, hi = self.escape()
                    if kind != "chr":
                        raise self.error("class escape as a range endpoint")
                if ord(c) > 0x7F or ord(hi) > 0x7F:
                    raise self.error("class range with a non-ASCII endpoint")
                if ord(hi) < ord(c):
                    raise self.error(f"reversed class range {c}-{hi}")
                ascii_set |= set(range(ord(c), ord(hi) + 1))
            elif ord(c) > 0x7F:
                wide.append(c)
            else:
                ascii_set.add(ord(c))
        if negate and neg_escapes:
            # [^\D...]: what every negated escape excludes, minus the rest
            keep = set(_ASCII)
            for val in neg_escapes:
                keep &= val
            return _codepoint(frozenset(keep - ascii_set), False)
        if negate:
            node = _codepoint(_ASCII - ascii_set, not wide)
            if wide:  # every multi-byte code point but the listed ones
                lo = 0x80
                for cp in sorted({ord(ch) for ch in wide}) + [0x110000]:
                    if lo <= cp - 1:
                        node[1].extend(_seq([range(a, b + 1) for a, b in sq])
                                       for sq in _utf8_ranges(lo, cp - 1))
                    lo = cp + 1
            return node
        for val in neg_escapes:  # e.g. [\D] : all but digits, any code point
            ascii_set |= _ASCII - val
        node = _codepoint(frozenset(ascii_set), bool(neg_escapes))
        if not neg_escapes:
            node[1].extend(_literal(ch) for ch in dict.fromkeys(wide))
        return node


def _utf8_ranges(lo: int, hi: int) -> list[list[tuple[int, int]]]:
    """Code points lo..hi (>= 0x80) as byte-range sequences: each entry is
    one (low, high) pair per byte. Surrogates are left out."""
    out: list[list[tuple[int, int]]] = []

    def split(lo: int, hi: int) -> None:
        if lo > hi:
            return
        for cut in (0x7FF, 0xD7FF, 0xDFFF, 0xFFFF):
            if lo <= cut < hi:
                split(lo, cut)
                split(cut + 1, hi)
                return
        if 0xD800 <= lo and hi <= 0xDFFF:
            return
        for i in (1, 2, 3):
            m = (1 << (6 * i)) - 1
            if lo & ~m != hi & ~m:
                if lo & m:
                    split(lo, lo | m)
                    split((lo | m) + 1, hi)
                    return
                if hi & m != m:
                    split(lo, (hi & ~m) - 1)
                    split(hi & ~m, hi)
                    return
        out.append(list(zip(chr(lo).encode("utf-8"), chr(hi).encode("utf-8"))))

    split(lo, hi)
    return out


class _NFA:
    def __init__(self, limit: int):
        self.eps: list[list[int]] = []
        self.edges: list[list[tuple[frozenset, int]]] = []
        self.limit = limit

    def new(self) -> int:
        if len(self.eps) >= self.limit:
            raise ValueError(
                f"grammar too large: more than {self.limit} NFA states")
        self.eps.append([])
        self.edges.append([])
        return len(self.eps) - 1

    @staticmethod
    def _sep_list(items: list, i: int, loops: list[int]) -> int:
        """m > 0 when items[i:i+m] is followed by (sep items[i:i+m])*."""
        for j in loops:
            m = j - i
            if m >= 1:
                inner = items[j][1][1]
                if len(inner) >= m and inner[len(inner) - m:] == items[i:j]:
                    return m
        return 0

    def build(self, node, start: int) -> int:
        """Add `node` starting at `start`; returns its end state."""
        kind = node[0]
        if kind == "set":
            end = self.new()
            if node[1]:
                self.edges[start].append((node[1], end))
            return end
        if kind == "cat":
            items = node[1]
            loops = [j for j, c in enumerate(items)
                     if c[0] == "rep" and c[2] == 0 and c[3] is None
                     and c[1][0] == "cat"]
            i = 0
            while i < len(items):
                m = self._sep_list(items, i, loops)
                if not m:
                    start = self.build(items[i], start)
                    i += 1
                    continue
                # X(sep X)* with X = items[i:i+m]: one copy of X, entered
                # again after sep. Separated lists (JSON arrays, objects)
                # would otherwise double their DFA states per nesting level.
                inner = items[i + m][1][1]
                head = self.new()
                self.eps[start].append(head)
                start = self.build(("cat", items[i:i + m]), head)
                back = self.build(("cat", inner[:len(inner) - m]), start)
                self.eps[back].append(head)
                i += m + 1
            return start
        if kind == "alt":
            end = self.new()
            for child in node[1]:
                s = self.new()
                self.eps[start].append(s)
                self.eps[self.build(child, s)].append(end)
            return end
        _, child, lo, hi = node
        for _ in range(lo):
            start = self.build(child, start)
        if hi is None:
            loop = self.new()
            self.eps[start].append(loop)
            self.eps[self.build(child, loop)].append(loop)
            return loop
        end = self.new()
        self.eps[start].append(end)
        for _ in range(hi - lo):
            s = self.new()
            self.eps[start].append(s)
            start = self.build(child, s)
            self.eps[start].append(end)
        return end


class DFA:
    """trans[s] maps a byte to the next state; state 0 is the start."""

    def __init__(self, trans: list[dict[int, int]], accepting: list[bool]):
        self.trans = trans
        self.accepting = accepting

    @property
    def num_states(self) -> int:
        return len(self.trans)

    def fullmatch(self, data: bytes) -> bool:
        s = 0
        for b in data:
            s = self.trans[s].get(b, -1)
            if s < 0:
                return False
        return self.accepting[s]

    def longest(self) -> int | None:
        """Length in bytes of the longest sentence, None if unbounded."""
        memo: dict[int, int] = {}
        on_path: set[int] = set()
        stack = [(0, iter(set(self.trans[0].values())))]
        on_path.add(0)
        best = {0: 0}
        while stack:
            s, it = stack[-1]
            for n in it:
                if n in on_path:
                    return None
                if n in memo:
                    best[s] = max(best[s], memo[n] + 1)
                    continue
                on_path.add(n)
                best[n] = 0
                stack.append((n, iter(set(self.trans[n].values()))))
                break
            else:
                stack.pop()
                on_path.discard(s)
                memo[s] = best[s]
                if stack:
                    p = stack[-1][0]
                    best[p] = max(best[p], memo[s] + 1)
        return memo[0]


def compile_regex(pattern: str, max_states: int = 20000) -> DFA:
    if not isinstance(pattern, str):
        raise ValueError("regex must be a string")
    ast = _Parser(pattern).parse()
    nfa = _NFA(limit=max(16 * max_states, 1024))
    start = nfa.new()
    final = nfa.build(ast, start)

    closure_memo: dict[int, frozenset] = {}

    def closure(states) -> frozenset:
        out: set[int] = set()
        for s0 in states:
            c = closure_memo.get(s0)
            if c is None:
                seen = {s0}
                todo = [s0]
                while todo:
                    for n in nfa.eps[todo.pop()]:
                        if n not in seen:
                            seen.add(n)
                            todo.append(n)
                c = closure_memo[s0] = frozenset(seen)
            out |= c
        return frozenset(out)

    ids = {closure([start]): 0}
    order = [closure([start])]
    trans: list[dict[int, int]] = []
    k = 0
    while k < len(order):
        by_byte: dict[int, set[int]] = {}
        for s in order[k]:
            for bset, tgt in nfa.edges[s]:
                for b in bset:
                    by_byte.setdefault(b, set()).add(tgt)
        row: dict[int, int] = {}
        memo: dict[frozenset, int] = {}
        for b, tgts in by_byte.items():
            key = frozenset(tgts)
            d = memo.get(key)
            if d is None:
                cl = closure(key)
                d = ids.get(cl)
                if d is None:
                    if len(order) >= max_states:
                        raise ValueError(
                            f"grammar too large: more than {max_states} DFA "
                            "states (structured_max_states)")
                    d = ids[cl] = len(order)
                    order.append(cl)
                memo[key] = d
            row[b] = d
        trans.append(row)
        k += 1
    accepting = [final in st for st in order]

    # trim: keep states that can reach an accepting state
    rev: list[list[int]] = [[] for _ in trans]
    for s, row in enumerate(trans):
        for n in set(row.values()):
            rev[n].append(s)
    live = {s for s, a in enumerate(accepting) if a}
    todo = list(live)
    while todo:
        for p in rev[todo.pop()]:
            if p not in live:
                live.add(p)
                todo.append(p)
    live.add(0)  # an empty language keeps a lone dead start state
    remap = {s: i for i, s in enumerate(sorted(live))}
    new_trans = [
        {b: remap[n] for b, n in trans[s].items() if n in live}
        for s in sorted(live)
    ]
    if not any(accepting):
        new_trans = [{}]
    return DFA(new_trans, [accepting[s] for s in sorted(live)])


def escape_literal(text: str) -> str:
    """`text` as a pattern of this dialect that matches exactly itself."""
    return "".join("\\" + c if c in _META else c for c in text)
