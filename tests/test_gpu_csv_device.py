"""Device CSV parser (``csv.hip`` + ``har.data.csv_device``) against the independent oracle of
``_csv_util``: the corpus of ``tests/test_csv_differential.py`` through ``parse_csv_device``.

Kinds, ints, double bit patterns, missing masks and strings of ``to_table()`` and of
``to_device_table()`` must equal the oracle's; ``dictionary_encode`` must order a vocabulary like
``StringIndexer`` (frequency descending, ties by ascending string), a quoted and an unquoted
spelling of one string being ONE value (the host parsers return the unquoted text of both); and the
line index is checked on its own for the files built around the 4096-byte workgroup chunk."""
from collections import Counter

import numpy as np
import pytest
import torch

from _csv_util import assert_table_matches, boundary_cases, corpus, line_index, structure_cases

pytestmark = pytest.mark.gpu

CASES = corpus()
LINE_CASES = boundary_cases() + [c for c in structure_cases() if c.name.startswith(("bom", "blank", "crlf", "lf"))]


@pytest.mark.parametrize("case", LINE_CASES, ids=[c.name for c in LINE_CASES])
def test_line_spans_match_python_index(cuda, case):
    from har.data.csv_device import _line_spans

    buf = torch.frombuffer(bytearray(case.raw), dtype=torch.uint8).to(cuda)
    starts, ends = _line_spans(buf, 3 if case.raw[:3] == b"\xef\xbb\xbf" else 0)
    want_s, want_e = line_index(case.raw)
    assert starts.cpu().tolist() == want_s
    assert ends.cpu().tolist() == want_e


@pytest.fixture(scope="module")
def parsed(cuda):
    """Every corpus file parsed once on the device, shared by the tests below."""
    from har.data.csv_device import parse_csv_device

    return {c.name: parse_csv_device(c.raw, cuda, header=c.header) for c in CASES}


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_to_table_matches_oracle(parsed, case):
    assert_table_matches(parsed[case.name].to_table(), case, "device")


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_to_device_table_matches_oracle(parsed, case):
    from har.data.table import DeviceColumn

    t = parsed[case.name].to_device_table()
    assert all(isinstance(t[n], DeviceColumn) for n in t.columns)
    for e in case.expected:  # the resident planes themselves, not only their host materialization
        col = t[e.name]
        if e.kind in ("int", "long"):
            assert col.tensor.dtype == torch.int64
            np.testing.assert_array_equal(col.tensor.cpu().numpy(), e.data, err_msg=f"{case.name}.{e.name}")
        elif e.kind == "double":
            assert col.tensor.dtype == torch.float64
            np.testing.assert_array_equal(col.tensor.cpu().numpy().view(np.int64), e.data.view(np.int64),
                                          err_msg=f"{case.name}.{e.name}")
        if e.kind != "string":
            np.testing.assert_array_equal(col.missing_t.cpu().numpy(), e.missing, err_msg=f"{case.name}.{e.name}")
    assert_table_matches(t, case, "device table")


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_dictionary_encode_order_and_counts(parsed, case):
    d = parsed[case.name]
    for e in case.expected:
        if e.kind != "string":
            continue
        freq = Counter(v for v in e.data if v is not None)
        want = sorted(freq, key=lambda s: (-freq[s], s))
        codes, vocab, counts = d.dictionary_encode(e.name)
        assert vocab == want, f"{case.name}.{e.name}"
        assert counts.tolist() == [freq[s] for s in want], f"{case.name}.{e.name}"
        c = codes.cpu().numpy()
        got = [None if k < 0 else vocab[k] for k in c]
        assert got == list(e.data), f"{case.name}.{e.name}"


def test_dictionary_case_has_ties_and_mixed_spellings():
    """What the two dictionary columns are there for (a property of the corpus, checked once)."""
    case = next(c for c in CASES if c.name == "dictionary")
    tie = Counter(next(e for e in case.expected if e.name == "tie").data)
    assert sorted(tie.values(), reverse=True)[:4] == [2, 2, 2, 2]
    assert b'\nb,ab,' in case.raw and b',"ab",' in case.raw
    mix = Counter(next(e for e in case.expected if e.name == "mix").data)
    assert mix["ab"] == 3 and mix["cd"] == 2 and mix[""] == 1 and mix[None] == 1
