"""Every traversal launcher of launch.h has a row in tests/wide_matrix.py, the row lists the staging
forms the launcher's definition branches on, and each form names a GPU parity test that runs it in
the wide accel mode (stack class 0).  No GPU: the sources are read as text."""
import os
import re

import pytest

from test_option_coverage import DEV, ROOT, _functions, _read
from wide_matrix import WIDE_MATRIX

FORMS = ("lds", "top", "plain")


def _launchers(text):
    """The launch_* templates declared in launch.h, in order."""
    return re.findall(r"template <int STK>\s*\nvoid (launch_\w+)\(", text)


def _bodies():
    """launcher -> the text of its definition in inst_pt.hip / inst_bd.hip, with the helpers it
    forwards to (launch_shadow_q_ns) appended."""
    src = _read(DEV, "inst_pt.hip") + _read(DEV, "inst_bd.hip")
    defs = {m.group(1): m.group(2) for m in
            re.finditer(r"\nvoid (launch_\w+)\([^)]*\) \{\n(.*?)\n\}\n", src, re.S)}
    out = {}
    for name, body in defs.items():
        for other, b in defs.items():
            if other != name and re.search(r"\b" + other + r"<", body):
                body += b
        out[name] = body
    return out


def _forms(body):
    """Staging forms a launcher's definition selects between: TOP by TravLaunch::top (or the `top`
    argument of launch_trace), LDS by TravLaunch::lds; every launcher has the plain form."""
    top = bool(re.search(r"\bl\.top\b|\bif \(top\)|LUMO_TRAV_LAUNCH_TOP\(", body))
    lds = bool(re.search(r"\bl\.lds\b|LUMO_TRAV_LAUNCH(_TOP)?\(", body))
    return {f for f, has in (("lds", lds), ("top", top), ("plain", True)) if has}


def test_rows_are_the_launchers():
    names = _launchers(_read(DEV, "launch.h"))
    assert names and len(set(names)) == len(names), names
    assert list(WIDE_MATRIX) == names
    # each is also instantiated for class 0 (LUMO_EXTERN_STK lists every launcher once)
    macro = re.search(r"#define LUMO_EXTERN_STK\(K\)(.*?)#ifndef LUMO_STK", _read(DEV, "launch.h"), re.S).group(1)
    assert re.findall(r"extern template void (launch_\w+)<K>", macro) == names
    assert "LUMO_EXTERN_STK(0)" in _read(DEV, "launch.h")


def test_rows_list_the_forms_of_the_definitions():
    bodies = _bodies()
    for name, row in WIDE_MATRIX.items():
        assert name in bodies, name
        assert set(row) == _forms(bodies[name]), (name, sorted(row), sorted(_forms(bodies[name])))
        assert set(row) <= set(FORMS)
    # the launchers kernels.hip asks a TOP form of (launch_trav's allow_top argument, and lumo_trace)
    kernels = _read(DEV, "kernels.hip")
    asked = set()
    for m in re.finditer(r"launch_trav\(", kernels):
        depth, k = 0, m.end() - 1
        while True:  # the call's closing parenthesis
            depth += {"(": 1, ")": -1}.get(kernels[k], 0)
            if depth == 0:
                break
            k += 1
        call = kernels[m.start():k + 1]
        named = re.findall(r"(launch_\w+)<decltype", call)
        if not named:  # launch_trav's own definition
            continue
        last = call[call.rindex("}") + 1:-1].split(",")  # the arguments after the lambda: stream, allow_top
        if named and len(last) >= 3 and last[2].strip() not in ("", "false"):
            asked.add(named[0])
    asked.add("launch_trace")
    assert asked == {n for n, row in WIDE_MATRIX.items() if "top" in row}, sorted(asked)


@pytest.mark.parametrize("name", list(WIDE_MATRIX))
def test_launcher_forms_have_wide_tests(name):
    for form, where in WIDE_MATRIX[name].items():
        path, fn = where.split("::")
        assert os.path.basename(path).startswith("test_gpu_wide"), where
        funcs = _functions(path)
        assert fn in funcs, where
        assert re.search(r"\baccel\b", funcs[fn]), f"{where} ({name}, {form}) does not name accel"
