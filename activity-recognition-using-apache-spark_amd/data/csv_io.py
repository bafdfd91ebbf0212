"""CSV ingest with Spark-compatible schema inference.

Replaces ``sqlContext.read.format('com.databricks.spark.csv').options(header='true',
inferschema='true').load(path)`` (``Main/main.py:18-20``).

Inference rule (per column, over non-empty fields): every field an integer
literal -> ``int`` (``long`` if it overflows int32); every field a decimal/float
literal -> ``double``; otherwise ``string``.  On WISDM this yields UID ``int``,
XAVG ``int`` (all zeros), ``*PEAK`` ``string`` (``?`` markers) and ``double`` for
the rest — the schema printed at ``result.txt:3-18``.

The byte-level work (line index, field split, number parse, type votes) runs in
the native multi-threaded parser ``csrc/host/csv_parser.cpp`` when the extension
is built; a pure-Python parser with identical semantics is the fallback and the
test oracle.  For device-resident ETL of very large numeric CSVs see
``har.ops.csv_device`` (HIP kernels K1/K2).
"""
from __future__ import annotations

import re
from typing import List, Optional, Tuple

import numpy as np

from .table import Column, Table

_INT_RE = re.compile(r"[+-]?[0-9]+\Z")
_FLOAT_RE = re.compile(r"[+-]?(?:(?:[0-9]+\.?[0-9]*|\.[0-9]+)(?:[eE][+-]?[0-9]+)?|NaN|Infinity)\Z")

INT32_MAX = 2 ** 31 - 1
INT32_MIN = -(2 ** 31)
INT64_MAX = 2 ** 63 - 1
INT64_MIN = -(2 ** 63)


def _split_line(line: str) -> List[Tuple[str, bool]]:
    """Fields ``(text, quoted)`` of one line — ``split_line`` of ``csrc/host/csv_parser.cpp``: a field
    that starts with ``"`` runs to its closing quote (``""`` escapes one), whatever follows up to the
    next comma is dropped; a trailing comma adds one empty field."""
    if '"' not in line:
        return [(f, False) for f in line.split(",")]
    out, i, e = [], 0, len(line)
    while True:
        if i < e and line[i] == '"':
            j, buf = i + 1, []
            while j < e:
                if line[j] == '"':
                    if j + 1 < e and line[j + 1] == '"':
                        buf.append('"')
                        j += 2
                        continue
                    break
                buf.append(line[j])
                j += 1
            out.append(("".join(buf), True))
            i = line.find(",", j + 1)
        else:
            k = line.find(",", i)
            out.append((line[i:e if k < 0 else k], False))
            i = k
        if i < 0 or i >= e:
            break
        i += 1  # skip ','
        if i == e:
            out.append(("", False))
            break
    return out


def _columns_from_fields(header: List[str], rows: List[List[Tuple[str, bool]]]) -> Table:
    cols = []
    for j, name in enumerate(header):
        cells = [r[j] if j < len(r) else ("", False) for r in rows]
        fields = [t for t, _ in cells]
        present = [q or t != "" for t, q in cells]  # a quoted "" is a present, empty string
        nonempty = [c for c, p in zip(cells, present) if p]
        miss = np.array([not p for p in present], dtype=bool)
        ints = None
        if nonempty and all(not q and _INT_RE.match(t) for t, q in nonempty):
            ints = [int(f) if p else 0 for f, p in zip(fields, present)]
            if not all(INT64_MIN <= v <= INT64_MAX for v in ints):
                ints = None  # an integer literal that does not fit a long: the column is a double
        if ints is not None:
            vals = np.array(ints, dtype=np.int64)
            kind = "int" if (vals.max() <= INT32_MAX and vals.min() >= INT32_MIN) else "long"
            cols.append(Column(name, kind, vals, miss if miss.any() else None))
        elif nonempty and all(not q and _FLOAT_RE.match(t) for t, q in nonempty):
            vals = np.array([float(f) if p else np.nan for f, p in zip(fields, present)], dtype=np.float64)
            cols.append(Column(name, "double", vals, miss if miss.any() else None))
        else:
            cols.append(Column(name, "string", np.array([f if p else None for f, p in zip(fields, present)],
                                                        dtype=object)))
    return Table(cols)


def parse_csv_text_python(text: str, header: bool = True) -> Table:
    """Line based like the native parser: every ``\\n`` ends a record (one ``\\r`` before it is
    dropped), empty lines are skipped, a UTF-8 BOM is ignored."""
    if text[:1] == "\ufeff":
        text = text[1:]
    lines = [ln[:-1] if ln.endswith("\r") else ln for ln in text.split("\n")]
    rows = [_split_line(ln) for ln in lines if ln]
    if not rows:
        return Table()
    if header:
        names, rows = [t.strip(" ") for t, _ in rows[0]], rows[1:]
    else:
        names = [f"_c{i}" for i in range(len(rows[0]))]
    return _columns_from_fields(names, rows)


def _native():
    try:
        from ..ops._native import host_module
        return host_module()
    except Exception:  # pragma: no cover - extension not built
        return None


def parse_csv_bytes(buf: bytes, header: bool = True, use_native: Optional[bool] = None) -> Table:
    mod = _native() if use_native in (None, True) else None
    if mod is None:
        if use_native:
            raise RuntimeError("native CSV parser requested but the extension is not built")
        return parse_csv_text_python(buf.decode("utf-8"), header=header)
    res = mod.csv_parse(buf, bool(header), 0)
    names = res["names"]
    cols = []
    for j, name in enumerate(names):
        kind = res["kinds"][j]
        miss = res["missing"][j]
        miss = miss if miss.any() else None
        if kind in ("int", "long"):
            cols.append(Column(name, kind, res["ints"][j], miss))
        elif kind == "double":
            cols.append(Column(name, "double", res["doubles"][j], miss))
        else:
            cols.append(Column(name, "string", np.asarray(res["strings"][j], dtype=object)))
    return Table(cols)


def read_csv(path: str, header: bool = True, infer_schema: bool = True,
             use_native: Optional[bool] = None, device=None, resident: bool = True) -> Table:
    """Load a CSV file into a columnar :class:`Table`.  ``device="cuda"`` parses on the
    GPU (``har.data.csv_device``: HIP line index + field parse + dictionary encoding) and,
    with ``resident``, keeps every column in HBM (:class:`DeviceColumn`: the feature pipeline
    then runs on the device); ``resident=False`` returns the equivalent host table."""
    if device is not None and str(device).startswith("cuda"):
        from .csv_device import read_csv_device

        d = read_csv_device(path, device=device, header=header)
        t = d.to_device_table() if (resident and infer_schema) else d.to_table()
    else:
        with open(path, "rb") as f:
            buf = f.read()
        t = parse_csv_bytes(buf, header=header, use_native=use_native)
    if not infer_schema:  # Spark without inferSchema: every column is a string
        t = Table([Column(c.name, "string", np.asarray([c.cell_str(i) for i in range(len(c))], dtype=object))
                   for c in (t[n] for n in t.columns)])
    return t
