"""Regular expressions for Reader.find_regex / count_regex / grep: a parser, and a compiler to the
deterministic automaton that kolm_find_dfa_device / kolm_reader_find_dfa walk on the device
(csrc/findrx_core.h, k_findrx.hip).

compile(expr, ignore_case) accepts a subset of Python's bytes `re` syntax in which every accepted
expression describes the language re.compile(expr, re.DOTALL [| re.IGNORECASE]) describes:

    everything kolm.classes.compile accepts: literal bytes, ., [...], \\d \\D \\w \\W \\s \\S, \\xHH,
        \\n \\r \\t \\f \\v \\0, backslash + punctuation or white space
    x* x+ x?  x{m} x{m,} x{,n} x{m,n}      after any atom or group
    x*? x+? x?? x{m,n}?                    the lazy forms: the same language
    a|b                                    alternation
    ( ... )  (?: ... )                     groups (nothing is captured: only starts are reported)

Refused with a ValueError that names the offset in the expression: the anchors ^ $ \\b \\B \\A \\Z,
back-references, every (? group but (?: (look-around, inline flags, names, atomic groups), the
possessive forms x*+ x++ x?+ x{m,n}+, a repeat of a repeat, octal escapes, a { that begins no
repeat (write \\{), and any expression that matches the empty string (every position would be a
match; the offset named is 0).

What a search reports: position o is a match of expression i iff some data[o:o + k], 1 <= k <= 256
and o + k <= end of the window, is matched by the expression exactly, which is
    re.compile(b"(?:" + expr + b")", flags).match(data, o, min(end, o + 256)) is not None.
Match lengths are not reported: greedy, lazy and leftmost-longest differ there, the set of starts
does not.

The automaton of a call (table(), Table): one class map and one transition table for all its
expressions.  Bytes whose columns are identical share a class; state 0 is dead, state 1 accepts and
is absorbing (every transition into a subset that holds an accepting position becomes 1, which is
what makes "some prefix matches" a walk that stops at the first accept); rows 0 and 1 are zero;
every expression has a start state >= 2.  A call holds at most MAX_ENTRIES = states x classes
transitions.  The subset construction stops as soon as that bound cannot be met any more, and
so does the unrolling of {m,n}: (a|b)*a(a|b){20} is refused after a few thousand subsets, not after
2^20.  States from which no accept is reachable are merged into the dead state."""
import re as _re
from typing import List, Optional, Sequence

import numpy as np

from . import classes
from .classes import ClassPattern, fold_class

MAX_PATTERNS = 16      # KOLM_FIND_MAX_PATTERNS
MAX_ENTRIES = 16384    # KOLM_RX_MAX_ENTRIES
MAX_WALK = 256         # KOLM_FIND_MAX_LEN: bytes of the longest witness

_ALL = frozenset(range(256))
_MAX_POSITIONS = 2 * MAX_ENTRIES  # NFA states of a call: an unrolled repeat stops here
_REPEAT = _re.compile(rb"\{(\d*)(?:(,)(\d*))?\}")


class _TooBig(ValueError):
    pass


def _too_big(what: str) -> _TooBig:
    return _TooBig(f"{what}: the automaton of a call holds at most {MAX_ENTRIES} transitions (states x byte classes)")


class _Parser:
    """expr -> a tree of ("set", frozenset), ("cat", [..]), ("alt", [..]), ("rep", node, m, n or None)."""

    def __init__(self, expr: bytes, ignore_case: bool):
        self.expr, self.i, self.ignore_case = expr, 0, ignore_case

    def error(self, at: int, what: str) -> ValueError:
        return ValueError(f"{what} at offset {at} of {self.expr!r}: not in the syntax of kolm.regex")

    def peek(self) -> int:
        return self.expr[self.i] if self.i < len(self.expr) else -1

    def parse(self):
        node = self.alt()
        if self.i < len(self.expr):  # only a ) stops alt()
            raise self.error(self.i, "a ) that closes nothing")
        return node

    def alt(self):
        branches = [self.cat()]
        while self.peek() == ord("|"):
            self.i += 1
            branches.append(self.cat())
        return branches[0] if len(branches) == 1 else ("alt", branches)

    def cat(self):
        items = []
        while self.i < len(self.expr) and self.expr[self.i] not in b"|)":
            items.append(self.repeat(self.atom()))
        return items[0] if len(items) == 1 else ("cat", items)

    def class_part(self, fn, at):
        try:
            return fn(self.expr, at)
        except ValueError as e:  # kolm.classes words its refusals for class patterns
            raise ValueError(str(e).split(": a class pattern")[0] + ": not in the syntax of kolm.regex") from None

    def atom(self):
        expr, at = self.expr, self.i
        c = expr[at]
        if c == ord("("):
            self.i += 1
            if self.peek() == ord("?"):
                if expr[self.i:self.i + 2] != b"?:":
                    raise self.error(at, "a group that begins with (? and is no (?: group (look-around, flags, names "
                                         "and atomic groups have no place here)")
                self.i += 2
            node = self.alt()
            if self.peek() != ord(")"):
                raise self.error(at, "an unterminated (")
            self.i += 1
            return node
        if c in b"*+?":
            raise self.error(at, f"'{chr(c)}' with nothing to repeat in front of it")
        if c == ord("{"):
            raise self.error(at, "a { with nothing to repeat in front of it (write \\{)")
        if c in b"^$":
            raise self.error(at, f"the anchor '{chr(c)}'")
        neg = False
        if c == ord("."):
            cl, self.i = _ALL, at + 1
        elif c == ord("["):
            cl, neg, self.i = self.class_part(classes._bracket, at)
        elif c == ord("\\"):
            nxt = expr[at + 1:at + 2]
            if nxt and nxt in b"bBAZ":
                raise self.error(at, f"the anchor \\{nxt.decode()}")
            if nxt and nxt in b"123456789":
                raise self.error(at, "a back-reference or octal escape")
            cl, self.i = self.class_part(classes._escape, at)
        else:
            cl, self.i = c, at + 1
        cl = frozenset({cl}) if isinstance(cl, int) else frozenset(cl)
        if self.ignore_case:
            cl = fold_class(cl)
        return ("set", _ALL - cl if neg else cl)

    def repeat(self, node):
        at, c = self.i, self.peek()
        if c == ord("*"):
            m, n, self.i = 0, None, at + 1
        elif c == ord("+"):
            m, n, self.i = 1, None, at + 1
        elif c == ord("?"):
            m, n, self.i = 0, 1, at + 1
        elif c == ord("{"):
            q = _REPEAT.match(self.expr, at)
            if not q or (not q.group(1) and not q.group(3)):
                raise self.error(at, "a { that begins no {m}, {m,}, {,n} or {m,n} (write \\{)")
            m = int(q.group(1) or 0)
            n = m if not q.group(2) else int(q.group(3)) if q.group(3) else None
            if n is not None and n < m:
                raise self.error(at, "a repeat whose maximum is below its minimum")
            if max(m, n or 0) > _MAX_POSITIONS:
                raise _too_big(f"the repeat at offset {at} of {self.expr!r}")
            self.i = q.end()
        else:
            return node
        if self.peek() == ord("?"):  # lazy: the same language
            self.i += 1
        elif self.peek() == ord("+"):
            raise self.error(self.i, "a possessive repeat")
        if self.peek() in (ord("*"), ord("+"), ord("?"), ord("{")):
            raise self.error(self.i, "a repeat of a repeat")
        return ("rep", node, m, n)


class _Nfa:
    """Thompson's construction over byte sets; every build() adds at least one state, so the
    bound on the states also bounds the work of an unrolled repeat."""

    def __init__(self):
        self.eps: List[List[int]] = []
        self.on: List[Optional[tuple]] = []  # (set id, target)
        self.accept: set = set()
        self.sets: List[frozenset] = []
        self._ids = {}

    def new(self) -> int:
        if len(self.eps) >= _MAX_POSITIONS:
            raise _too_big(f"the expressions unroll to more than {_MAX_POSITIONS} positions")
        self.eps.append([])
        self.on.append(None)
        return len(self.eps) - 1

    def set_id(self, s: frozenset) -> int:
        if s not in self._ids:
            self._ids[s] = len(self.sets)
            self.sets.append(s)
        return self._ids[s]

    def build(self, node):
        kind = node[0]
        if kind == "set":
            s, e = self.new(), self.new()
            self.on[s] = (self.set_id(node[1]), e)
            return s, e
        if kind == "cat":
            s = cur = self.new()
            for it in node[1]:
                a, b = self.build(it)
                self.eps[cur].append(a)
                cur = b
            return s, cur
        if kind == "alt":
            s, e = self.new(), self.new()
            for br in node[1]:
                a, b = self.build(br)
                self.eps[s].append(a)
                self.eps[b].append(e)
            return s, e
        _, sub, m, n = node
        s = cur = self.new()
        for _ in range(m):
            a, b = self.build(sub)
            self.eps[cur].append(a)
            cur = b
        if n is None:
            loop = self.new()
            a, b = self.build(sub)
            self.eps[cur].append(loop)
            self.eps[loop].append(a)
            self.eps[b].append(loop)
            return s, loop
        e = self.new()
        for _ in range(n - m):
            a, b = self.build(sub)
            self.eps[cur] += [a, e]
            cur = b
        self.eps[cur].append(e)
        return s, e

    def closure(self, s: int, memo: dict) -> frozenset:
        """The states reachable from s without reading a byte that read one or accept."""
        if s not in memo:
            seen, stack = {s}, [s]
            while stack:
                for t in self.eps[stack.pop()]:
                    if t not in seen:
                        seen.add(t)
                        stack.append(t)
            memo[s] = frozenset(t for t in seen if self.on[t] is not None or t in self.accept)
        return memo[s]


class Table:
    """The automaton of a call.  cls_map: 256 bytes, the class of every byte value; T: the
    transitions as a (nstates, ncls) uint16 array; starts: the start state of every expression."""
    __slots__ = ("cls_map", "T", "starts", "nstates", "ncls", "_rows")

    def __init__(self, cls_map: bytes, T: np.ndarray, starts: Sequence[int]):
        self.cls_map, self.T, self.starts = bytes(cls_map), np.ascontiguousarray(T, np.uint16), list(starts)
        self.nstates, self.ncls = self.T.shape
        self._rows = self.T.tolist()

    @property
    def entries(self) -> int:
        return self.nstates * self.ncls

    def matches(self, data: bytes, o: int, end: Optional[int] = None, i: int = 0) -> bool:
        """The walk of csrc/findrx_core.h for expression i from offset o of data[:end]."""
        end = len(data) if end is None else end
        rows, s = self._rows, self.starts[i]
        for k in range(o, min(end, o + MAX_WALK)):
            s = rows[s][self.cls_map[data[k]]]
            if s <= 1:
                break
        return s == 1


def _build_table(trees, what) -> Table:
    nfa = _Nfa()
    starts = []
    try:
        for t in trees:
            s, e = nfa.build(t)
            starts.append(s)
            nfa.accept.add(e)
    except RecursionError:
        raise ValueError(f"{what}: groups nested too deeply") from None
    # bytes that no set of the call tells apart read alike
    sig = {}
    byte_cls = [sig.setdefault(tuple(b in s for s in nfa.sets), len(sig)) for b in range(256)]
    ncls = len(sig)
    rep = [byte_cls.index(c) for c in range(ncls)]
    has = [[rep[c] in s for c in range(ncls)] for s in nfa.sets]
    memo: dict = {}
    index, subsets, rows = {}, [None, None], [[0] * ncls, [0] * ncls]

    def state_of(sub: frozenset) -> int:
        if not sub:
            return 0
        if sub & nfa.accept:
            return 1
        k = index.get(sub)
        if k is None:
            k = index[sub] = len(subsets)
            subsets.append(sub)
            rows.append(None)
            # the pruning below removes states, the merge of columns classes: neither can save a
            # table that is already four times too large
            if len(subsets) * ncls > 4 * MAX_ENTRIES:
                raise _too_big(f"{what} need more than {len(subsets)} states x {ncls} classes")
        return k

    start_state = []
    for i, s in enumerate(starts):
        sub = nfa.closure(s, memo)
        if sub & nfa.accept:
            raise ValueError(f"expression {i} of {what} matches the empty string at offset 0: every position would "
                             "be a match")
        start_state.append(state_of(sub) if sub else None)
    k = 2
    while k < len(subsets):
        row = []
        for c in range(ncls):
            nxt = set()
            for s in subsets[k]:
                tr = nfa.on[s]
                if tr is not None and has[tr[0]][c]:
                    nxt |= nfa.closure(tr[1], memo)
            row.append(state_of(frozenset(nxt)))
        rows[k] = row
        k += 1
    # states that cannot reach the accept are the dead state
    back = [[] for _ in rows]
    for s in range(2, len(rows)):
        for t in set(rows[s]):
            back[t].append(s)
    live, stack = {1}, [1]
    while stack:
        for s in back[stack.pop()]:
            if s not in live:
                live.add(s)
                stack.append(s)
    # renumber what the starts reach; a start that reaches no accept (an empty class) keeps a
    # state of its own with a row of zeros
    order, number = [], {0: 0, 1: 1}
    stack = []
    for i, s in enumerate(start_state):
        if s is None or s not in live:
            start_state[i] = -1 - i
            number[-1 - i] = 2 + len(order)
            order.append(None)
        elif s not in number:
            number[s] = 2 + len(order)
            order.append(s)
            stack.append(s)
    while stack:
        for t in rows[stack.pop()]:
            if t in live and t not in number:
                number[t] = 2 + len(order)
                order.append(t)
                stack.append(t)
    T = np.zeros((2 + len(order), ncls), np.uint16) if 2 + len(order) <= 0xFFFF else None
    if T is None:
        raise _too_big(f"{what} need {2 + len(order)} states")
    for new, s in enumerate(order, 2):
        if s is not None:
            T[new] = [number[t] if t in live else 0 for t in rows[s]]
    # bytes with identical columns share a class
    cols, final = {}, []
    for c in range(ncls):
        final.append(cols.setdefault(T[:, c].tobytes(), len(cols)))
    keep = [final.index(c) for c in range(len(cols))]
    T = np.ascontiguousarray(T[:, keep])
    if T.shape[0] * T.shape[1] > MAX_ENTRIES:
        raise _too_big(f"{what} need {T.shape[0]} states x {T.shape[1]} classes")
    return Table(bytes(final[byte_cls[b]] for b in range(256)), T, [number[s] for s in start_state])


class Regex:
    """One compiled expression.  `.expr`: the source (None for Regex.literal / of_classes);
    `.ignore_case`; `.table`: its own automaton (a search compiles one for all its expressions:
    table()); `.host`: the compiled `re` object that means the same."""
    __slots__ = ("expr", "ignore_case", "tree", "table", "host", "_classes")

    def __init__(self, tree, expr, ignore_case, host_expr, class_sets=None):
        what = repr(expr) if expr is not None else "the pattern"
        object.__setattr__(self, "tree", tree)
        object.__setattr__(self, "expr", expr)
        object.__setattr__(self, "ignore_case", bool(ignore_case))
        object.__setattr__(self, "_classes", class_sets)
        object.__setattr__(self, "table", _build_table([tree], what))
        flags = _re.DOTALL | (_re.IGNORECASE if ignore_case and expr is not None else 0)
        object.__setattr__(self, "host", _re.compile(b"(?:" + host_expr + b")", flags))

    def __setattr__(self, name, value):
        raise AttributeError("Regex is immutable")

    def __repr__(self):
        return f"Regex({self.expr if self.expr is not None else self.host.pattern!r}, ignore_case={self.ignore_case})"

    @classmethod
    def of_classes(cls, pattern: ClassPattern) -> "Regex":
        """The class pattern as an expression: a concatenation of its classes."""
        tree = ("cat", [("set", c) for c in pattern.classes])
        return cls(tree, None, False, pattern.regex(), pattern.classes)

    @classmethod
    def literal(cls, b, ignore_case: bool = False) -> "Regex":
        """The bytes b (ASCII letters in either case with ignore_case)."""
        return cls.of_classes(ClassPattern.literal(b, ignore_case))

    def folded(self) -> "Regex":
        """This expression with ignore_case."""
        if self.ignore_case:
            return self
        if self.expr is not None:
            return compile(self.expr, True)
        return Regex.of_classes(ClassPattern(fold_class(c) for c in self._classes))


def compile(expr, ignore_case: bool = False) -> Regex:  # noqa: A001 (as re.compile)
    """The Regex of `expr` (see the module's text); ValueError for what is not accepted."""
    expr = memoryview(expr).tobytes()
    try:
        tree = _Parser(expr, ignore_case).parse()
    except RecursionError:
        raise ValueError(f"{expr!r}: groups nested too deeply") from None
    return Regex(tree, expr, ignore_case, expr)


def as_regex(p, ignore_case: bool = False) -> Regex:
    """A Regex as it is (ignore_case folds it), a ClassPattern converted, an expression compiled."""
    if isinstance(p, Regex):
        return p.folded() if ignore_case else p
    if isinstance(p, ClassPattern):
        return Regex.of_classes(classes.as_pattern(p, ignore_case))
    return compile(p, ignore_case)


def as_list(exprs, ignore_case: bool = False) -> List[Regex]:
    """One expression, Regex or ClassPattern, or a sequence of them, as a list of Regex."""
    if isinstance(exprs, (bytes, bytearray, memoryview, Regex, ClassPattern)):
        exprs = [exprs]
    return [as_regex(p, ignore_case) for p in exprs]


def table(regexes: Sequence[Regex]) -> Table:
    """The one automaton of a call's expressions (1..MAX_PATTERNS): a shared class map and table,
    a start state each."""
    regexes = list(regexes)
    if not 1 <= len(regexes) <= MAX_PATTERNS:
        raise ValueError(f"{len(regexes)} expressions (1..{MAX_PATTERNS} are allowed)")
    if len(regexes) == 1:
        return regexes[0].table
    return _build_table([r.tree for r in regexes], f"the {len(regexes)} expressions")
