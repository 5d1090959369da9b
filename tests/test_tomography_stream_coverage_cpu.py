"""``include/aogym_tomography.h`` held to the rule ``test_stream_coverage_cpu.py`` holds ``include/aogym.h`` to: every entry point it declares with
a ``void* stream`` has a place in ``COVERED`` of ``test_gpu_tomography_streams.py`` (with the test there that drives it on a caller's stream) or
in its ``NOT_DRIVEN`` (with the reason), and ``NOT_DRIVEN`` holds nothing that a public Python method calls."""
import ast
import os

from test_stream_coverage_cpu import ROOT, _python_callers, stream_entry_points


def _tables():
    with open(os.path.join(ROOT, "tests", "test_gpu_tomography_streams.py")) as f:
        tree = ast.parse(f.read())
    found, tests = {}, set()
    for node in tree.body:
        if isinstance(node, ast.Assign) and len(node.targets) == 1 and isinstance(node.targets[0], ast.Name) and node.targets[0].id in ("COVERED", "NOT_DRIVEN"):
            found[node.targets[0].id] = ast.literal_eval(node.value)
        if isinstance(node, ast.FunctionDef) and node.name.startswith("test_"):
            tests.add(node.name)
    return found["COVERED"], found["NOT_DRIVEN"], tests


def _problems(text):
    names = stream_entry_points(text)
    covered, not_driven, tests = _tables()
    lines = []
    if not names or len(names) != len(set(names)):
        lines.append(f"the header parse found {len(names)} names, {len(set(names))} distinct")
    lines += [f"{n}: in COVERED and in NOT_DRIVEN" for n in set(covered) & set(not_driven)]
    lines += [f"{n}: an entry point with a stream parameter that test_gpu_tomography_streams.py places nowhere" for n in names
              if n not in covered and n not in not_driven]
    lines += [f"{n}: placed, but not (or no longer) declared with a stream parameter" for n in list(covered) + list(not_driven) if n not in names]
    lines += [f"{n}: COVERED names {t}, which test_gpu_tomography_streams.py does not define" for n, t in covered.items() if t not in tests]
    for n, reason in not_driven.items():
        if not (isinstance(reason, str) and reason.strip()):
            lines.append(f"{n}: NOT_DRIVEN gives no reason")
        if _python_callers(n):
            lines.append(f"{n} is in NOT_DRIVEN but {_python_callers(n)} call it: drive it on a side stream")
    return lines


def _header():
    with open(os.path.join(ROOT, "include", "aogym_tomography.h")) as f:
        return f.read()


def test_the_header_declares_the_stream_entry_points():
    assert stream_entry_points(_header()) == ["aog_wavefront_project", "aog_tomo_upload", "aog_tomo_update", "aog_tomo_reset", "aog_tomo_get_state",
                                              "aog_tomo_set_state"]


def test_every_stream_entry_point_is_placed():
    lines = _problems(_header())
    assert not lines, "\n".join(lines)


def test_a_new_stream_entry_point_is_reported():
    lines = _problems(_header() + "\nint aog_z(aog_tomo*,\n          void* stream);\n")
    assert lines == ["aog_z: an entry point with a stream parameter that test_gpu_tomography_streams.py places nowhere"]


def test_the_python_callers_are_found():
    assert "tomography.py" in _python_callers("aog_wavefront_project")
    for name in ("aog_tomo_upload", "aog_tomo_update", "aog_tomo_reset", "aog_tomo_get_state", "aog_tomo_set_state"):
        assert _python_callers(name), name
