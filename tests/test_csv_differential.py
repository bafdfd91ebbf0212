"""Host CSV parsers (native C++ and pure Python) against the independent oracle of ``_csv_util``.

Every corpus file goes through both parsers; kinds, ints, the bit patterns of doubles (so that
``-0.0`` and NaN count), missing masks and strings must equal what the oracle derives from the
cells the file was built from.  No GPU is involved."""
import numpy as np
import pytest

from _csv_util import I64_MAX, NON_NUMBERS, assert_table_matches, corpus, infer_column, line_index

from har.data.csv_io import parse_csv_bytes

CASES = corpus()


def _native_built():
    try:
        from har.ops._native import host_module
        return host_module() is not None
    except Exception:
        return False


@pytest.mark.parametrize("use_native", [True, False], ids=["native", "python"])
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_host_parser_matches_oracle(case, use_native):
    if use_native:
        assert _native_built(), "the native extension is not built (build() compiles it)"
    table = parse_csv_bytes(case.raw, header=case.header, use_native=use_native)
    assert_table_matches(table, case, "native" if use_native else "python")


def test_corpus_covers_what_it_claims():
    """The generator's own promises: chunk-boundary bytes, sizes, kinds reached, no case dropped."""
    by = {c.name: c for c in CASES}
    assert sum(c.name.startswith("random_") for c in CASES) == 20
    for p in (4095, 4096, 4097):
        assert by[f"lf_at_{p}"].raw[p:p + 1] == b"\n"
    assert by["crlf_straddles_chunk"].raw[4095:4097] == b"\r\n"
    assert len(by["len_4096"].raw) == 4096 and len(by["len_8192"].raw) == 8192
    assert len(by["forty_kb"].raw) >= 10 * 4096
    tok = {e.name: e for e in by["tokens"].expected}
    assert tok["fast_long"].kind == "long" and 9007199254740993 in tok["fast_long"].data
    assert tok["ext_long"].kind == "long" and I64_MAX in tok["ext_long"].data
    assert tok["ext_big"].kind == "double" and tok["fast_big"].kind == "double"
    assert tok["spec_double"].kind == "double" and tok["sign_int"].kind == "int"
    assert all(tok[f"non_{i}"].kind == "string" for i in range(len(NON_NUMBERS)))
    assert all(e.kind == "double" for n, e in tok.items() if n.endswith("_mix"))
    kinds = {e.kind for c in CASES if c.name.startswith("random_") for e in c.expected}
    assert kinds == {"int", "long", "double", "string"}


def test_oracle_rule_examples():
    """The oracle itself on hand-computed examples (it is the reference of three parsers)."""
    e = infer_column("a", [("9223372036854775807", False), ("", False), ("-1", False)])
    assert e.kind == "long" and list(e.data) == [2 ** 63 - 1, 0, -1] and list(e.missing) == [False, True, False]
    e = infer_column("a", [("9223372036854775808", False), ("1", False)])
    assert e.kind == "double" and list(e.data) == [9223372036854775808.0, 1.0]
    e = infer_column("a", [("1", False), ("", True)])
    assert e.kind == "string" and list(e.data) == ["1", ""]
    e = infer_column("a", [("", False), None])
    assert e.kind == "string" and list(e.data) == [None, None]
    e = infer_column("a", [("-0", False), ("-0.", False)])
    assert e.kind == "double" and np.signbit(e.data[0]) and np.signbit(e.data[1])  # float("-0") is -0.0
    assert line_index(b"\xef\xbb\xbfa\r\n\r\nb\n\nc") == ([3, 8, 11], [4, 9, 12])
