"""Every execution option has a row in tests/option_matrix.py, the row's range is the one ctx.hip's
option table (kOpts) accepts, and the row names a GPU parity test that renders with the option away
from its default (or says why none does).  No GPU: the sources are read as text."""
import ast
import os
import re

import pytest

from lumo_amd import _ffi
from option_matrix import OPTION_MATRIX, STACK_CLASSES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = os.path.join(ROOT, "lumo_amd", "csrc", "device")
EXEMPT = {"timing", "poison"}


def _read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


def _const(text, name):
    m = re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*(\d+)\s*;", text)
    assert m, name
    return int(m.group(1))


def _kopts():
    """kOpts of ctx.hip: [(LUMO_OPT_* name, environment variable, lo, hi)] in table order."""
    state = _read(DEV, "state.h")
    names = {"BLOCK": _const(state, "BLOCK"), "MAX_MERGE": _const(state, "MAX_MERGE"),
             "SNAP_RING": _const(_read(DEV, "ctx.h"), "SNAP_RING")}
    src = _read(DEV, "ctx.hip")
    body = re.search(r"constexpr OptDef kOpts\[\] = \{(.*?)\n\};", src, re.S)
    assert body
    rows = re.findall(r'\{\s*(LUMO_OPT_\w+)\s*,\s*"(LUMO_\w+)"\s*,\s*&Opts::\w+\s*,\s*([^,{}]+?)\s*,\s*([^,{}]+?)\s*\}',
                      body.group(1))

    def val(expr):
        e = expr.replace("(int64_t)", "").replace("Ctx::", "")
        assert re.fullmatch(r"[\w\s<>/*+\-()]+", e), expr
        return int(eval(e, {"__builtins__": {}}, names))  # integer constants and the three names above only

    return [(n, env, val(lo), val(hi)) for n, env, lo, hi in rows]


def test_rows_are_the_options():
    assert list(OPTION_MATRIX) == list(_ffi.OPTIONS)


def test_ranges_are_ctx_hips():
    rows = _kopts()
    assert len(rows) == len(_ffi.OPTIONS)
    header = _read(ROOT, "include", "lumo_amd.h")
    enum = re.findall(r"^\s*(LUMO_OPT_[A-Z_]+)\b(?: = 0)?,", header, re.M)
    assert [r[0] for r in rows] == enum[:len(rows)]  # table order = enum order = _ffi.OPTIONS order
    for name, (opt, env, lo, hi) in zip(_ffi.OPTIONS, rows):
        row = OPTION_MATRIX[name]
        assert row.lo == lo, (name, row.lo, lo)
        if row.hi is None:  # the device's LDS per CU at run time; the table holds MI355X's 160 KiB
            assert name == "top_kb" and hi == 160
        else:
            assert row.hi == hi, (name, row.hi, hi)
        if row.values is not None:
            assert min(row.values) == lo and max(row.values) == hi, name
        if row.default is not None:
            assert lo <= row.default <= hi, name
    assert OPTION_MATRIX["stack_class"].values == (0,) + STACK_CLASSES
    m = re.search(r"STACK_CLASSES\[\]\s*=\s*\{([^}]*)\}", _read(DEV, "launch.h"))
    assert tuple(int(x) for x in m.group(1).split(",")) == STACK_CLASSES


def test_header_states_the_ranges():
    """The header comment of each option gives the bounds the table accepts (the form the comments
    use: `lo-hi`, `a / b / c` or `0 / 1`; powers of two as 2^k)."""
    header = _read(ROOT, "include", "lumo_amd.h")
    body = header[header.index("LUMO_OPT_TIMING = 0"):header.index("LUMO_OPT_COUNT")]
    parts = re.split(r"\n\s*(?=LUMO_OPT_)", body)
    assert len(parts) == len(_ffi.OPTIONS)

    def show(v):
        return f"2^{v.bit_length() - 1}" if v >= 1 << 16 and v & (v - 1) == 0 else str(v)

    for name, text in zip(_ffi.OPTIONS, parts):
        row = OPTION_MATRIX[name]
        text = " ".join(text.split())
        if row.values is not None:
            want = [" / ".join(str(v) for v in row.values if v != 0)]
        elif (row.lo, row.hi) == (0, 1):
            want = ["0 / 1"]
        elif row.hi is None:
            want = ["0 to the CU's LDS"]
        else:  # a range, its special low values (-1 / 0: auto, off) listed apart in some comments
            want = [f"{lo}-{show(row.hi)}" for lo in (row.lo, 0, 1) if lo >= row.lo]
        each = row.hi is not None and row.hi - row.lo <= 3 and all(  # `-1 auto, 0 off, 1 ..., 2 ...`
            re.search(r"(?<![\w.^])" + re.escape(str(v)) + r"(?![\w.])", text) for v in range(row.lo, row.hi + 1))
        assert each or any(w in text for w in want), (name, want, text)


def _functions(path):
    tree = ast.parse(_read(ROOT, path))
    src = _read(ROOT, path).splitlines()
    return {n.name: "\n".join(src[n.lineno - 1:n.end_lineno]) for n in tree.body if isinstance(n, ast.FunctionDef)}


@pytest.mark.parametrize("name", _ffi.OPTIONS)
def test_option_has_a_parity_test(name):
    row = OPTION_MATRIX[name]
    if row.exempt:
        assert name in EXEMPT and row.exempt.startswith(name + ":")
        return
    assert name not in EXEMPT
    assert row.covered, f"{name}: no GPU test renders with it set"
    for value, where in row.covered:
        assert value != row.default and row.lo <= value and (row.hi is None or value <= row.hi), (name, value)
        if row.values is not None:
            assert value in row.values
        path, fn = where.split("::")
        assert os.path.basename(path).startswith("test_gpu_")
        funcs = _functions(path)
        assert fn in funcs, where
        assert re.search(r"\b" + name + r"\b", funcs[fn]), f"{where} does not name {name}"
