"""CSV corpus and an independent oracle for the differential parser tests.

Nothing here imports the code under test.  Every corpus file is *constructed* from a grid of
cells ``(text, quoted)`` (``None`` = the row ends before this column), so the expected columns
come from the cells and the documented inference rule, never from parsing the bytes back:

* a field is missing when it is empty and unquoted (or its row is too short);
* a column whose non-empty fields are all integer literals within int64 is ``int`` (``long``
  beyond int32), its values ``int(text)``;
* a column whose non-empty fields are all float literals (integer literals included, those
  outside int64 too) is ``double``, each value ``float(text)`` and NaN where missing;
* anything else (a quoted field, however numeric it looks, included) is ``string``; a quoted
  empty field is a present empty string, an unquoted one is ``None``;
* a column without any non-empty field is ``string``.

Both parsers under test are line based by design: a newline always ends a record and whatever
follows a closing quote up to the next comma is dropped.  The generator therefore never emits a
newline inside a quoted field nor junk after a closing quote.
"""
from __future__ import annotations

import random
import re
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

CHUNK = 4096  # bytes per workgroup of the device line index

_INT = re.compile(r"[+-]?[0-9]+\Z")
_FLOAT = re.compile(r"[+-]?(?:(?:[0-9]+\.?[0-9]*|\.[0-9]+)(?:[eE][+-]?[0-9]+)?|NaN|Infinity)\Z")
I64_MIN, I64_MAX = -(2 ** 63), 2 ** 63 - 1
I32_MIN, I32_MAX = -(2 ** 31), 2 ** 31 - 1

Cell = Optional[Tuple[str, bool]]  # (text, quoted) or None when the row has no such field
MISSING: Cell = ("", False)


class Expected(NamedTuple):
    name: str
    kind: str
    data: np.ndarray               # int64 | float64 | object (str / None)
    missing: Optional[np.ndarray]  # bool mask (numeric kinds), None for strings


class CsvCase(NamedTuple):
    name: str
    raw: bytes
    header: bool
    expected: List[Expected]
    nrows: int


def U(text: str) -> Cell:
    return (text, False)


def Q(text: str) -> Cell:
    return (text, True)


# ---------------------------------------------------------------------------------- the oracle
def infer_column(name: str, cells: Sequence[Cell]) -> Expected:
    text = [("" if c is None else c[0]) for c in cells]
    quoted = [(c is not None and c[1]) for c in cells]
    present = [q or t != "" for t, q in zip(text, quoted)]
    nonempty = [(t, q) for t, q, p in zip(text, quoted, present) if p]
    miss = np.array([not p for p in present], dtype=bool)
    if nonempty and all(not q and _INT.match(t) for t, q in nonempty):
        ints = [int(t) if p else 0 for t, p in zip(text, present)]
        if all(I64_MIN <= v <= I64_MAX for v in ints):
            kind = "int" if all(I32_MIN <= v <= I32_MAX for v in ints) else "long"
            return Expected(name, kind, np.array(ints, dtype=np.int64), miss)
    if nonempty and all(not q and _FLOAT.match(t) for t, q in nonempty):
        vals = np.array([float(t) if p else float("nan") for t, p in zip(text, present)], dtype=np.float64)
        return Expected(name, "double", vals, miss)
    return Expected(name, "string", np.array([t if p else None for t, p in zip(text, present)], dtype=object), None)


def line_index(raw: bytes) -> Tuple[List[int], List[int]]:
    """[b, e) of every non-empty line (BOM skipped, one CR stripped) — plain Python."""
    b = 3 if raw[:3] == b"\xef\xbb\xbf" else 0
    starts, ends = [], []
    n = len(raw)
    while b <= n:
        e = raw.find(b"\n", b)
        if e < 0:
            e = n
        x = e - 1 if e > b and raw[e - 1:e] == b"\r" else e
        if x > b:
            starts.append(b)
            ends.append(x)
        b = e + 1
    return starts, ends


# ---------------------------------------------------------------------------------- the builder
def _field(c: Cell) -> str:
    text, quoted = c
    if quoted:
        return '"' + text.replace('"', '""') + '"'
    assert not any(ch in text for ch in ',"\r\n'), text
    return text


def build_case(name: str, names: Sequence[str], columns: Sequence[Sequence[Cell]], *, header: bool = True,
               eol: str = "\n", final_newline: bool = True, bom: bool = False, blank_after: Sequence[int] = (),
               trailing_blank: int = 0, extra: Optional[dict] = None, trailing_comma: Sequence[int] = ()) -> CsvCase:
    """One file from column-major cells.  ``columns[j][r] is None`` means row r stops before column
    j (every later column of that row must be None too).  ``extra[r]`` appends fields beyond the
    header (ignored by every parser); ``trailing_comma`` rows end in a bare comma (one more empty
    field); ``blank_after`` inserts an empty line after those rows (-1 = after the header)."""
    ncol = len(names)
    nrows = len(columns[0]) if columns else 0
    assert all(len(c) == nrows for c in columns)
    lines = []
    if header:
        lines.append(",".join(names))
    else:
        names = [f"_c{j}" for j in range(ncol)]
        assert nrows and all(col[0] is not None for col in columns), "the first row fixes the column count"
    if -1 in blank_after:
        lines.append("")
    for r in range(nrows):
        fields = []
        for j in range(ncol):
            c = columns[j][r]
            if c is None:
                assert all(columns[k][r] is None for k in range(j, ncol))
                break
            fields.append(_field(c))
        fields += [_field(c) for c in (extra or {}).get(r, ())]
        line = ",".join(fields) + ("," if r in trailing_comma else "")
        assert line != "", "an empty line would be dropped as blank"
        lines.append(line)
        if r in blank_after:
            lines.append("")
    body = eol.join(lines) + (eol if final_newline else "") + eol * trailing_blank
    raw = (b"\xef\xbb\xbf" if bom else b"") + body.encode("utf-8")
    expected = [infer_column(n, col) for n, col in zip(names, columns)]
    return CsvCase(name, raw, header, expected, nrows)


def _pad(cols: List[List[Cell]]) -> List[List[Cell]]:
    n = max(len(c) for c in cols)
    return [list(c) + [MISSING] * (n - len(c)) for c in cols]


# ---------------------------------------------------------------------------------- token table
SIGN_DOT = ["0", "-0", "+5", "1.", ".5", "-.5e-3", "1e5", "1E+05"]
FAST_PATH = ["1e22", "1e23", "1e-22", "1e-23", "123456789012345678", "1234567890123456789",
             "1.234567890123456789", "1234567890123456789012345", "0.1234567890123456789012345",
             "0." + "0" * 30 + "123", "0" * 25, "9007199254740992", "9007199254740993"]
EXTREMES = ["2147483647", "2147483648", "-2147483649", "9223372036854775807", "-9223372036854775808",
            "9223372036854775808", "4.9e-324", "1e-400", "1e400", "1e4294967296", "1e-4294967297"]
SPECIALS = ["NaN", "+NaN", "Infinity", "-Infinity"]
NON_NUMBERS: List[Cell] = [U("Infected"), U("infinity"), U("nan"), U("1e"), U("e5"), U("."), U("-"), U("+"),
                           U("1.2.3"), Q("1,"), U("0x10"), U("1_000"), U("1d"), U(" 1"), Q("")]
FAMILIES = {"sign": SIGN_DOT, "fast": FAST_PATH, "ext": EXTREMES, "spec": SPECIALS}
NUMERIC_TOKENS = SIGN_DOT + FAST_PATH + EXTREMES + SPECIALS


def _own_kind(tok: str) -> str:
    if _INT.match(tok):
        v = int(tok)
        return "int" if I32_MIN <= v <= I32_MAX else "long" if I64_MIN <= v <= I64_MAX else "big"
    return "double"


def token_case() -> CsvCase:
    """Every token in a column of its own kind and mixed into a double column.  A numeric family
    splits into an int, a long, a beyond-int64 and a float column; every non-number gets a column
    of its own between two doubles (it alone must turn that column into a string)."""
    names, cols = [], []
    for fam, toks in FAMILIES.items():
        for kind in ("int", "long", "big", "double"):
            own = [U(t) for t in toks if _own_kind(t) == kind]
            if own:
                names.append(f"{fam}_{kind}")
                cols.append(own)
        mixed: List[Cell] = []
        for i, t in enumerate(toks):
            mixed += [U(t), U(f"{i}.25")]
        names.append(f"{fam}_mix")
        cols.append(mixed)
    names.append("non_all")
    cols.append(list(NON_NUMBERS))
    for i, c in enumerate(NON_NUMBERS):
        names.append(f"non_{i}")
        cols.append([U("1.5"), c, U("-2.5e3")])
    return build_case("tokens", names, _pad(cols))


# ---------------------------------------------------------------------------------- structure
def _small() -> Tuple[List[str], List[List[Cell]]]:
    return ["id", "x", "s", "q"], [
        [U("1"), U("2"), U("3"), U("40")],
        [U("0.5"), MISSING, U("-1e3"), U("7")],
        [U("ab"), Q("ab"), U("c d"), Q('say "hi"')],
        [Q("a,b"), Q(""), Q("x"), MISSING],
    ]


def structure_cases() -> List[CsvCase]:
    n, c = _small()
    out = [
        build_case("lf", n, c),
        build_case("crlf", n, c, eol="\r\n"),
        build_case("lf_nofinal", n, c, final_newline=False),
        build_case("crlf_nofinal", n, c, eol="\r\n", final_newline=False),
        build_case("bom", n, c, bom=True),
        build_case("bom_crlf", n, c, bom=True, eol="\r\n"),
        build_case("blank_mid", n, c, blank_after=(-1, 1)),
        build_case("blank_mid_crlf", n, c, blank_after=(0, 2), eol="\r\n"),
        build_case("blank_end", n, c, trailing_blank=3),
        build_case("blank_end_crlf", n, c, trailing_blank=2, eol="\r\n"),
        build_case("noheader", n, c, header=False),
        build_case("zero_rows", n, [[], [], [], []]),
        build_case("zero_rows_nofinal", n, [[], [], [], []], final_newline=False),
        build_case("one_row", n, [col[:1] for col in c]),
        build_case("one_col", ["v"], [[U("1"), U("-2"), U("3000000000")]]),
        build_case("one_col_one_row", ["v"], [[U("2.5")]], final_newline=False),
        build_case("one_col_noheader", ["v"], [[U("x"), U("y"), U("x")]], header=False),
    ]
    # ragged rows: row 1 has two fields only, row 2 carries two extra fields, row 0 and row 3 end in a comma
    # (row 3's comma fills the last column with an empty field, row 0's adds a field beyond the header)
    rag = [
        [U("1"), U("2"), U("3"), U("4"), U("5")],
        [U("1.5"), U("2.5"), U("x"), U("4.5"), MISSING],
        [U("7"), None, U("9"), U("10"), U("11")],
        [U("a"), None, Q("b,c"), None, None],
    ]
    out.append(build_case("ragged", ["a", "b", "c", "d"], rag, extra={2: (U("zz"), Q("y"))}, trailing_comma=(0,)))
    rag2 = [[U("1"), U("2"), U("3"), U("4")], [U("4"), U("5"), MISSING, None]]
    out.append(build_case("ragged_trailing_comma_fills", ["a", "b"], rag2, eol="\r\n"))
    # a quoted empty field is a present empty string: it turns an otherwise numeric column into a string
    qe = [[U("1"), U("2"), U("3")], [U("1.5"), Q(""), U("2.5")], [U("1"), MISSING, U("3")]]
    out.append(build_case("quoted_empty", ["i", "qe", "ue"], qe))
    # frequency ties (b == c, a == d) and quoted / unquoted spellings of one string
    tie = ["b", "a", "c", "b", "c", "a", "d", "d", "e"]
    mix: List[Cell] = [U("ab"), Q("ab"), U("cd"), Q("cd"), Q("ab"), U("ef"), Q("e,f"), MISSING, Q("")]
    out.append(build_case("dictionary", ["tie", "mix", "n"],
                          [[U(t) for t in tie], mix, [U(str(i)) for i in range(len(tie))]]))
    return out


# ---------------------------------------------------------------------------------- chunk boundaries
def _boundary_file(name: str, lf_at: Optional[int] = None, total: Optional[int] = None, eol: str = "\n",
                   final_newline: bool = True) -> CsvCase:
    """Header ``k,s,v``; the string column of row 1 is padded so that row 1's ``\\n`` lands on byte
    ``lf_at`` (with CRLF the ``\\r`` sits on ``lf_at - 1``), or the last row's so that the file is
    ``total`` bytes long."""
    names = ["k", "s", "v"]
    nrows = 6 if total is None else 40
    cols: List[List[Cell]] = [[U(str(i)) for i in range(nrows)], [U(f"r{i}") for i in range(nrows)],
                              [U(f"{i}.5") for i in range(nrows)]]
    probe = build_case(name, names, cols, eol=eol, final_newline=final_newline)
    if lf_at is not None:
        row, want = 1, lf_at
        have = probe.raw.index(eol.encode() * 1, probe.raw.index(b"1,r1,")) + len(eol) - 1
    else:
        row, want, have = nrows - 1, total, len(probe.raw)
    assert want > have
    cols[1][row] = U(cols[1][row][0] + "p" * (want - have))
    case = build_case(name, names, cols, eol=eol, final_newline=final_newline)
    if lf_at is not None:
        assert case.raw[lf_at:lf_at + 1] == b"\n" and (eol == "\n" or case.raw[lf_at - 1:lf_at] == b"\r")
    else:
        assert len(case.raw) == total
    return case


def boundary_cases() -> List[CsvCase]:
    out = [_boundary_file(f"lf_at_{p}", lf_at=p) for p in (CHUNK - 1, CHUNK, CHUNK + 1)]
    out.append(_boundary_file("crlf_straddles_chunk", lf_at=CHUNK, eol="\r\n"))
    out += [_boundary_file(f"len_{t}", total=t) for t in (CHUNK, 2 * CHUNK)]
    out += [_boundary_file(f"len_{t}_nofinal", total=t, final_newline=False) for t in (CHUNK, 2 * CHUNK)]
    # ~40 KB: the newline prefix scan spans ten workgroups and more
    n = 1800
    big = build_case("forty_kb", ["i", "x", "s"],
                     [[U(str(i * 7919)) for i in range(n)], [U(f"{i}.{i % 97:02d}e-2") for i in range(n)],
                      [U(f"label{i % 13}") for i in range(n)]], eol="\r\n")
    assert len(big.raw) >= 10 * CHUNK
    out.append(big)
    for n in (255, 256, 257):  # the lane tail of the one-lane-per-row parse
        out.append(build_case(f"rows_{n}", ["i", "x"], [[U(str(i - 128)) for i in range(n)],
                                                          [U(f"-{i}.125") for i in range(n)]]))
    return out


# ---------------------------------------------------------------------------------- seeded random files
def _random_decimal(rng: random.Random) -> str:
    nd = rng.randint(1, 20)
    digits = "".join(rng.choice("0123456789") for _ in range(nd))
    s = rng.choice(["", "", "-", "+"])
    form = rng.randrange(4)
    if form == 0:
        return s + digits
    cut = rng.randint(0, nd)
    body = digits[:cut] + "." + digits[cut:]
    if form == 3:
        body += rng.choice("eE") + rng.choice(["", "+", "-"]) + str(rng.randint(0, 30))
    return s + body


def random_cases(count: int = 20, seed: int = 20181) -> List[CsvCase]:
    rng = random.Random(seed)
    ints = [t for t in NUMERIC_TOKENS if _own_kind(t) in ("int", "long")]
    out = []
    for k in range(count):
        nrows, ncols = rng.randint(1, 300), rng.randint(1, 6)
        cols: List[List[Cell]] = []
        for j in range(ncols):
            flavour = rng.choice(["int", "long", "decimal", "token", "token+junk", "string"])
            col: List[Cell] = []
            for r in range(nrows):
                # (a one-column file cannot hold an empty field: the line would be blank)
                if ncols > 1 and rng.random() < 0.05:
                    col.append(MISSING)
                elif flavour == "int":
                    col.append(U(str(rng.randint(-10 ** 6, 10 ** 6))))
                elif flavour == "long":
                    col.append(U(rng.choice(ints) if rng.random() < 0.1 else str(rng.randint(-10 ** 18, 10 ** 18))))
                elif flavour == "decimal":
                    col.append(U(_random_decimal(rng)))
                elif flavour == "token":
                    col.append(U(rng.choice(NUMERIC_TOKENS) if rng.random() < 0.5 else _random_decimal(rng)))
                elif flavour == "token+junk":
                    col.append(rng.choice(NON_NUMBERS) if rng.random() < 0.02 else U(_random_decimal(rng)))
                else:
                    w = rng.choice(["walk", "jog", "sit", "up stairs", "a,b", 'q"q', ""])
                    col.append(Q(w) if (rng.random() < 0.3 or any(ch in w for ch in ',"') or w == "") else U(w))
            cols.append(col)
        header = rng.random() < 0.8
        out.append(build_case(f"random_{k}", [f"c{j}" for j in range(ncols)], cols, header=header,
                              eol=rng.choice(["\n", "\r\n"]), final_newline=rng.random() < 0.7))
    return out


_CORPUS: Optional[List[CsvCase]] = None


def corpus() -> List[CsvCase]:
    """The whole corpus, built once and shared (cases are immutable tuples)."""
    global _CORPUS
    if _CORPUS is None:
        _CORPUS = [token_case()] + structure_cases() + boundary_cases() + random_cases()
        assert len({c.name for c in _CORPUS}) == len(_CORPUS)
    return _CORPUS


# ---------------------------------------------------------------------------------- comparison
def assert_table_matches(table, case: CsvCase, what: str) -> None:
    """Kinds, ints, double bit patterns, missing masks and strings of a parsed Table vs the oracle."""
    exp = case.expected
    assert table.columns == [e.name for e in exp], f"{what} {case.name}: column names"
    if exp:
        assert table.count() == case.nrows, f"{what} {case.name}: {table.count()} rows, expected {case.nrows}"
    for e in exp:
        col = table[e.name]
        where = f"{what} {case.name}.{e.name}"
        assert col.kind == e.kind, f"{where}: kind {col.kind}, expected {e.kind}"
        data = np.asarray(col.data)
        if e.kind == "string":
            assert list(data) == list(e.data), where
            continue
        miss = np.zeros(case.nrows, dtype=bool) if col.missing is None else np.asarray(col.missing, dtype=bool)
        np.testing.assert_array_equal(miss, e.missing, err_msg=where + " missing mask")
        if e.kind == "double":
            assert data.dtype == np.float64, where
            np.testing.assert_array_equal(data.view(np.int64), e.data.view(np.int64), err_msg=where + " (bits)")
        else:
            assert data.dtype == np.int64, where
            np.testing.assert_array_equal(data, e.data, err_msg=where)
