"""Class patterns: fixed-length patterns whose positions are sets of bytes, for
Reader.find_classes / count_classes / grep and the ignore_case searches.

compile(expr, ignore_case) accepts a subset of Python's bytes `re` syntax in which every accepted
expression means exactly what re.compile(expr, re.DOTALL [| re.IGNORECASE]) means:

    a literal byte          that byte
    .                       any byte, newline included
    [...]                   ranges, a leading ^, a literal ] first, and the escapes below inside
    \\d \\D \\w \\W \\s \\S       ASCII, as for bytes patterns
    \\xHH  \\n \\r \\t \\f \\v \\0  the named byte
    \\ + punctuation         that punctuation byte (white space too: the output of re.escape)
    {k} after a class       k >= 1 copies of the class: still fixed length

Everything else raises ValueError with the offset in the expression: a class pattern is
fixed-length, so * + ? | ( ) ^ $, {m,n}, {0} and other backslash escapes have no place in it.

Case folding is ASCII only: fold(b) = b + 32 for A..Z, else b; the folded class is
{b : fold(b) in fold(C)}, and a negation is applied after the folding (re.IGNORECASE for bytes).

The library (csrc/findcls_core.h) sorts the classes of a call into masked equalities
{b : (b & mask) == value}, which count against no limit, and table classes, of which a call holds
at most 64 distinct ones; masked_equality() is the same rule in Python."""
import string
from typing import FrozenSet, Iterable, Optional, Tuple

MAX_LEN = 256          # KOLM_FIND_MAX_LEN
MAX_TABLE_CLASSES = 64  # KOLM_FIND_MAX_TABLE_CLASSES

_ALL = frozenset(range(256))
_DIGIT = frozenset(b"0123456789")
_WORD = frozenset(string.ascii_letters.encode() + b"0123456789_")
_SPACE = frozenset(b" \t\n\r\f\v")
_SHORTHAND = {ord("d"): _DIGIT, ord("D"): _ALL - _DIGIT, ord("w"): _WORD, ord("W"): _ALL - _WORD,
              ord("s"): _SPACE, ord("S"): _ALL - _SPACE}
_NAMED = {ord("n"): 10, ord("r"): 13, ord("t"): 9, ord("f"): 12, ord("v"): 11}
_PUNCT = frozenset(string.punctuation.encode() + b" \t\n\r\v\f")  # what re.escape puts a backslash before
_HEX = frozenset(b"0123456789abcdefABCDEF")
_VARIABLE = frozenset(b"*+?|()^$")


def fold(b: int) -> int:
    return b + 32 if 65 <= b <= 90 else b


def fold_class(c: Iterable[int]) -> FrozenSet[int]:
    """{b : fold(b) in fold(C)}: C closed under ASCII case."""
    f = {fold(b) for b in c}
    return frozenset(b for b in range(256) if fold(b) in f)


def masked_equality(c: Iterable[int]) -> Optional[Tuple[int, int]]:
    """(mask, value) when C == {b : (b & mask) == value}, else None (an empty or a table class)."""
    c = frozenset(c)
    if not c:
        return None
    v, o = 0xFF, 0
    for b in c:
        v &= b
        o |= b
    x = o ^ v
    return (~x & 0xFF, v) if len(c) == 1 << bin(x).count("1") else None


def _bitmap(c: FrozenSet[int]) -> bytes:
    bm = bytearray(32)
    for b in c:
        bm[b >> 3] |= 1 << (b & 7)
    return bytes(bm)


def _class_expr(c: FrozenSet[int]) -> bytes:
    """The class as an expression of \\xHH ranges."""
    if not c:
        return b"[^\\x00-\\xff]"
    out, b = [], 0
    while b < 256:
        if b in c:
            e = b
            while e + 1 in c:
                e += 1
            out.append(b"\\x%02x" % b if e == b else b"\\x%02x-\\x%02x" % (b, e))
            b = e
        b += 1
    return b"[" + b"".join(out) + b"]"


class ClassPattern:
    """An immutable sequence of 1..256 byte classes.  `.classes`: a tuple of frozensets of byte
    values; `.bitmaps`: the same as 32-byte bitmaps back to back (bit b & 7 of byte b >> 3), the
    form of the C ABI; len(): the positions."""
    __slots__ = ("classes", "bitmaps")

    def __init__(self, classes):
        cl = tuple(frozenset(c) for c in classes)
        if not 1 <= len(cl) <= MAX_LEN:
            raise ValueError(f"a class pattern has 1..{MAX_LEN} positions, not {len(cl)}")
        for c in cl:
            if not c <= _ALL:
                raise ValueError("a class holds byte values 0..255")
        object.__setattr__(self, "classes", cl)
        object.__setattr__(self, "bitmaps", b"".join(_bitmap(c) for c in cl))

    def __setattr__(self, name, value):
        raise AttributeError("ClassPattern is immutable")

    def __len__(self) -> int:
        return len(self.classes)

    def __eq__(self, other):
        return isinstance(other, ClassPattern) and self.classes == other.classes

    def __hash__(self):
        return hash(self.classes)

    def __repr__(self):
        return f"ClassPattern({self.regex()!r})"

    @classmethod
    def of(cls, sets) -> "ClassPattern":
        """From one set of byte values (or a 32-byte bitmap) per position."""
        out = []
        for s in sets:
            if isinstance(s, (bytes, bytearray)) and len(s) == 32:
                s = {b for b in range(256) if (s[b >> 3] >> (b & 7)) & 1}
            out.append(s)
        return cls(out)

    @classmethod
    def literal(cls, b, ignore_case: bool = False) -> "ClassPattern":
        """The bytes b, each position a single byte (an ASCII case pair with ignore_case)."""
        b = memoryview(b).tobytes()
        return cls([fold_class({x}) if ignore_case else {x} for x in b])

    def regex(self) -> bytes:
        """An expression of \\xHH classes that means this pattern to `re`."""
        return b"".join(_class_expr(c) for c in self.classes)


def _error(expr: bytes, at: int, what: str):
    return ValueError(f"{what} at offset {at} of {expr!r}: a class pattern is fixed-length "
                      "(literals, ., [...], \\d \\w \\s, \\xHH and {k} only)")


def _escape(expr: bytes, i: int):
    """The escape whose backslash is expr[i]: (class or byte value, the offset behind it)."""
    if i + 1 >= len(expr):
        raise _error(expr, i, "a lone backslash")
    c = expr[i + 1]
    if c in _SHORTHAND:
        return _SHORTHAND[c], i + 2
    if c in _NAMED:
        return _NAMED[c], i + 2
    if c == ord("x"):
        h = expr[i + 2:i + 4]
        if len(h) != 2 or not set(h) <= _HEX:
            raise _error(expr, i, "\\x needs two hex digits")
        return int(h, 16), i + 4
    if c == ord("0"):
        if i + 2 < len(expr) and expr[i + 2] in b"0123456789":
            raise _error(expr, i, "an octal escape")
        return 0, i + 2
    if c in _PUNCT:
        return c, i + 2
    raise _error(expr, i, f"the escape \\{chr(c) if 32 <= c < 127 else hex(c)}")


def _bracket(expr: bytes, i: int):
    """The class whose [ is expr[i], not folded and not negated: (set, negated, offset behind ])."""
    start = i
    i += 1
    neg = i < len(expr) and expr[i] == ord("^")
    if neg:
        i += 1
    out, first = set(), True
    while True:
        if i >= len(expr):
            raise _error(expr, start, "an unterminated [")
        c = expr[i]
        if c == ord("]") and not first:
            return out, neg, i + 1
        first = False
        at = i
        if c == ord("\\"):
            lo, i = _escape(expr, i)
        else:
            lo, i = c, i + 1
        if i + 1 < len(expr) and expr[i] == ord("-") and expr[i + 1] != ord("]"):
            if expr[i + 1] == ord("\\"):
                hi, j = _escape(expr, i + 1)
            else:
                hi, j = expr[i + 1], i + 2
            if not isinstance(lo, int) or not isinstance(hi, int) or hi < lo:
                raise _error(expr, at, "a bad range")
            out.update(range(lo, hi + 1))
            i = j
        elif isinstance(lo, int):
            out.add(lo)
        else:
            out |= lo


def _repeat(expr: bytes, i: int) -> Tuple[int, int]:
    """The {k} whose brace is expr[i]: (k, offset behind it)."""
    j = expr.find(b"}", i)
    body = expr[i + 1:j] if j > 0 else b""
    if not body.isdigit() or int(body) < 1:
        raise _error(expr, i, "a repeat other than {k} with k >= 1")
    return int(body), j + 1


def compile(expr, ignore_case: bool = False) -> ClassPattern:  # noqa: A001 (as re.compile)
    """The class pattern of `expr` (see the module's text); ValueError for what is not one."""
    expr = memoryview(expr).tobytes()
    if not expr:
        raise _error(expr, 0, "an empty expression")
    out, i, repeated = [], 0, True  # repeated: no class in front that a {k} could take
    while i < len(expr):
        c = expr[i]
        if c == ord("{"):
            if repeated:
                raise _error(expr, i, "a { with no class in front of it (write \\{)")
            k, i = _repeat(expr, i)
            if len(out) - 1 + k > MAX_LEN:
                raise ValueError(f"{expr!r} has more than {MAX_LEN} positions")
            out.extend([out[-1]] * (k - 1))
            repeated = True
            continue
        neg = False
        if c in _VARIABLE:
            raise _error(expr, i, f"'{chr(c)}'")
        if c == ord("."):
            cl, i = _ALL, i + 1
        elif c == ord("["):
            cl, neg, i = _bracket(expr, i)
        elif c == ord("\\"):
            cl, i = _escape(expr, i)
        else:
            cl, i = c, i + 1
        cl = frozenset({cl}) if isinstance(cl, int) else frozenset(cl)
        if ignore_case:
            cl = fold_class(cl)
        out.append(_ALL - cl if neg else cl)
        repeated = False
        if len(out) > MAX_LEN:
            raise ValueError(f"{expr!r} has more than {MAX_LEN} positions")
    return ClassPattern(out)


def as_pattern(p, ignore_case: bool = False) -> ClassPattern:
    """A ClassPattern as it is (ignore_case folds its classes), an expression compiled."""
    if isinstance(p, ClassPattern):
        return ClassPattern(fold_class(c) for c in p.classes) if ignore_case else p
    return compile(p, ignore_case)


def table_classes(patterns) -> int:
    """The distinct table classes of a call's patterns (the library allows MAX_TABLE_CLASSES)."""
    return len({c for p in patterns for c in p.classes if c and masked_equality(c) is None})
