#!/usr/bin/env python
"""What the library generates and says for a run-time-compiled objective, recorded once and committed
(tests/test_objective_sources_cpu.py holds every later build to it, byte for byte).

collect() asks the built library, through the lbfgsx_objective_source* entry points of include/lbfgsx.h, for
  sources   the generated translation unit of every form x {f64, f32} x every K the form accepts (and D for a mesh
            objective) x the optional second body {present, absent, empty string};
  refusals  the text of every refused request the entry points can make: an unknown dtype, the K and D next to the accepted
            ranges, a missing and an empty body, the word asm in either body;
  bind      what lbfgsx_objective_bind says to a handle of each of the four forms it does not bind.
The bodies are arbitrary text: nothing but the four handles of `bind` is compiled.  No GPU is needed.

    python tests/golden/make_objective_sources_golden.py        # writes tests/golden/objective_sources.json
"""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "objective_sources.json")

BODY = "const T u = x[0] * c[0];\ng[0] = u; // \"quoted\" \\ back\n\treturn T(0.5) * (u * x[0]);"
SECOND = "g[0] = p1[i] * x[0];\nreturn T(0.5) * (g[0] * x[0]);"
WORD = "as" + "m"
BAD = "%s volatile(\"\");\nreturn x[0];" % WORD
# form: (entry-point suffix, the arguments between dtype and the bodies for every accepted K (and D), has a second body,
#        the K / D arguments next to the accepted ranges)
FORMS = {
    "term": ("", [(1,), (2,)], False, [(0,), (3,)]),
    "chain": ("_chain", [(2,), (3,)], False, [(1,), (4,)]),
    "grid": ("_grid", [()], False, []),
    "graph": ("_graph", [()], True, []),
    "mesh": ("_mesh", [(K, D) for K in (2, 3, 4) for D in (1, 2, 3)], True, [(1, 2), (5, 2), (3, 0), (3, 4)]),
    "linear": ("_linear", [()], True, []),
}
SECONDS = {"present": SECOND.encode(), "absent": None, "empty": b""}


def _source(core, L, suffix, dtype, args, second, body, has_second):
    """(text, None) or (None, the refusal)"""
    fn = getattr(core, "lbfgsx_objective_source" + suffix)
    bodies = ((second, body) if has_second else (body,))
    need = fn(dtype, *args, *bodies, None, 0)
    if need < 0:
        assert need == L.E_INVALID
        return None, L.last_error()
    buf = C.create_string_buffer(int(need))
    assert fn(dtype, *args, *bodies, buf, need) == need
    return buf.value.decode(), None


def collect():
    sys.path.insert(0, ROOT)
    import numpy as np

    import lbfgspp_amd as A
    from lbfgspp_amd import _lib as L
    core, _ = A.load()
    out = {"sources": {}, "refusals": {}, "bind": {}}
    for form, (suffix, accepted, has_second, beside) in FORMS.items():
        def ask(dtype, args, second, body):
            return _source(core, L, suffix, dtype, args, second, body, has_second)
        for dname, dtype in (("f64", L.F64), ("f32", L.F32)):
            for args in accepted:
                for sname, second in (SECONDS.items() if has_second else [("none", None)]):
                    text, why = ask(dtype, args, second, BODY.encode())
                    assert why is None, why
                    out["sources"]["/".join([form, dname, "args=%s" % (list(args),), "second=" + sname])] = text
        good = accepted[-1]
        cases = [("dtype=7", 7, good, None, BODY.encode()), ("body=null", L.F64, good, None, None),
                 ("body=empty", L.F64, good, None, b""), ("body=%s" % WORD, L.F64, good, None, BAD.encode())]
        cases += [("args=%s" % (list(a),), L.F64, a, None, BODY.encode()) for a in beside]
        if has_second:
            cases.append(("second=%s" % WORD, L.F64, good, BAD.encode(), BODY.encode()))
        for cname, dtype, args, second, body in cases:
            text, why = ask(dtype, args, second, body)
            assert text is None, (form, cname)
            out["refusals"][form + "/" + cname] = why
    # lbfgsx_objective_bind refuses these four by the handle's form, before it looks at the context: any non-null pointer
    # stands for one here, so that no device is needed
    elem = "g[0] = x[0]; g[1] = x[1]; return x[0] * x[1];"
    handles = {"grid": A.GridObjective("g[0] = g[1] = g[2] = g[3] = x[0]; return x[0];", shape=(2, 2)),
               "graph": A.GraphObjective(elem, edges=(np.array([0]), np.array([1]))),
               "mesh": A.MeshObjective(elem, np.array([[0, 1]]), 1),
               "linear": A.LinearObjective("dz = z; return T(0.5) * (z * z);", _one_entry_matrix(np), 1)}
    placeholder = C.create_string_buffer(8)
    for form, f in handles.items():
        rc = core.lbfgsx_objective_bind(C.cast(placeholder, C.c_void_p), f.compile(), None, None, None)
        assert rc == L.E_INVALID
        out["bind"][form] = L.last_error()
    return out


def _one_entry_matrix(np):
    return (np.array([0, 1], np.int32), np.array([0], np.int32), np.array([1.0]))


def main():
    golden = collect()
    with open(OUT, "w") as f:
        json.dump(golden, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote %s (%d bytes): %d sources, %d refusals, %d bind refusals"
          % (OUT, os.path.getsize(OUT), len(golden["sources"]), len(golden["refusals"]), len(golden["bind"])))


if __name__ == "__main__":
    main()
