"""Every host-side counter of ``aog_env`` that feeds a device random stream or an episode position travels with the state blob: it stands in
the ``StateTail`` initialiser of ``aog_get_state`` and is assigned in ``aog_set_state`` (csrc/aogym.hip).  The names are listed here by hand,
each with its reason, and looked up in ``aogym_internal.h``: a new counter is added to ``COUNTERS`` (and to the tail, and gets its case in
test_gpu_checkpoint.py) or to ``NOT_STATE`` consciously.  A reminder, not a parser of C++."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "adaptive_optics_gym_amd", "csrc")

# member of aog_env -> why a resumed run needs it
COUNTERS = {
    "timestep": "the global step: the wind shift of a dynamic atmosphere and the extrusion's noise stream are functions of it",
    "rng_seed": "the key of every device Philox stream (screens, extrusion, Shack-Hartmann, detector, pyramid)",
    "sh_calls": "the Shack-Hartmann photon stream's call index",
    "steps_since_reset": "the episode position: when ``done`` is raised",
    "obs_frame": "the detector's frame: observations written so far",
    "pyr_frame": "the pyramid sensor's photon stream: sensor calls so far",
}
# counters of aog_env that evolve and are deliberately NOT simulation state -> why
NOT_STATE = {
    "sci_frames": "the science camera's frame count, with sci_exposure: measurement data that aog_set_state leaves as it was",
}


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _strip_comments(text):
    return re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))


def _body(text, head):
    """The brace-balanced body that follows the first match of ``head`` in ``text``."""
    m = re.search(head, text)
    assert m, f"{head!r} not found"
    i = text.index("{", m.end() - 1)
    depth, j = 0, i
    while True:
        depth += {"{": 1, "}": -1}.get(text[j], 0)
        if depth == 0:
            return text[i + 1:j]
        j += 1


def _members(text):
    """The names declared as members of ``struct aog_env`` with an integer type (comments stripped): good enough to find a counter."""
    body = _body(_strip_comments(text), r"struct\s+aog_env\s*\{")
    names = set()
    for m in re.finditer(r"\b(?:u?int\d+_t|int|unsigned(?:\s+long\s+long)?|long\s+long)\b\s*\*?\s*([^;()]*);", body):
        for decl in m.group(1).split(","):
            n = re.match(r"\s*\*?\s*(\w+)", decl)
            if n:
                names.add(n.group(1))
    return names


def _problems(internal_h, aogym_hip, counters):
    hip = _strip_comments(aogym_hip)
    members = _members(internal_h)
    init = re.search(r"StateTail\s*\{([^}]*)\}", _body(hip, r"\bint\s+aog_get_state\s*\([^)]*\)\s*\{"))
    setter = _body(hip, r"\bint\s+aog_set_state\s*\([^)]*\)\s*\{")
    lines = []
    if init is None:
        return ["aog_get_state: no StateTail{...} initialiser found"]
    for name in counters:
        if name not in members:
            lines.append(f"{name}: listed here, but no integer member of aog_env in aogym_internal.h")
        if not re.search(r"\be->" + name + r"\b", init.group(1)):
            lines.append(f"{name}: not in the StateTail initialiser of aog_get_state")
        if not re.search(r"\be->" + name + r"\s*=[^=]", setter):
            lines.append(f"{name}: not assigned in aog_set_state")
    return lines


def test_every_counter_travels_with_the_blob():
    lines = _problems(_read("aogym_internal.h"), _read("aogym.hip"), COUNTERS)
    assert not lines, "\n".join(lines)


def test_every_listed_name_has_a_reason_and_a_place():
    assert not set(COUNTERS) & set(NOT_STATE)
    members = _members(_read("aogym_internal.h"))
    for name, reason in list(COUNTERS.items()) + list(NOT_STATE.items()):
        assert isinstance(reason, str) and reason.strip(), f"{name}: no reason given"
        assert name in members, f"{name}: no integer member of aog_env"


def test_a_forgotten_counter_is_reported():
    """The check's own search: a counter that aog_get_state does not save, one that aog_set_state does not restore, and one that is not
    a member at all are each named."""
    hip = _read("aogym.hip")
    internal = _read("aogym_internal.h")
    assert "e->pyr_frame = tail.pyr_frame;" in hip and ", e->pyr_frame}" in hip
    lines = _problems(internal, hip.replace("e->pyr_frame = tail.pyr_frame;", ""), COUNTERS)
    assert lines == ["pyr_frame: not assigned in aog_set_state"]
    lines = _problems(internal, hip.replace(", e->pyr_frame}", "}"), COUNTERS)
    assert lines == ["pyr_frame: not in the StateTail initialiser of aog_get_state"]
    lines = _problems(internal, hip, dict(COUNTERS, new_counter="a stream someone adds"))
    assert lines == ["new_counter: listed here, but no integer member of aog_env in aogym_internal.h",
                     "new_counter: not in the StateTail initialiser of aog_get_state", "new_counter: not assigned in aog_set_state"]


def test_the_python_state_carries_its_mirrors():
    """``BatchedAOEnv.get_state`` names the Python-side mirrors of those counters, and ``set_state`` assigns each."""
    with open(os.path.join(ROOT, "adaptive_optics_gym_amd", "batched_env.py")) as f:
        text = f.read()
    getter = text[text.index("    def get_state(self):"):text.index("    def set_state(self, state):")]
    setter = text[text.index("    def set_state(self, state):"):text.index("    def accumulate_returns(")]
    for name in ("timestep", "episode_no", "observation_frames", "pyramid_frame_count"):
        assert re.search(r"\"" + name + r"\":\s*self\." + name + r"\b", getter), f"{name}: not in get_state's dictionary"
        assert re.search(r"self\." + name + r"\s*=\s*int\(state", setter), f"{name}: not assigned in set_state"
