"""The table of tests/streamcases.py checked without a GPU: it covers every
stream-taking Engine method, every poison is valid input of the real input's
dtype, shape and stride, and every poison changes the CPU reference's answer."""
import numpy as np
import pytest

import streamcases as SC

CPU_INPUTS = [n for n, c in SC.CASES.items() if not c.gpu_inputs]
CPU_REF = [n for n, c in SC.CASES.items() if c.ref is not None]


def test_every_stream_taking_method_is_covered():
    methods = SC.stream_methods()
    assert len(methods) >= 28
    assert len(SC.NOT_COVERED) <= 3 and all(isinstance(r, str) and r for r in SC.NOT_COVERED.values())
    groups = (set(SC.CASES), set(SC.CHAINED), set(SC.NOT_COVERED))
    assert sum(len(g) for g in groups) == len(set().union(*groups))
    assert sorted(set().union(*groups)) == methods
    # the forms whose inputs the GPU test has to render are checked there
    assert len(CPU_INPUTS) >= len(SC.CASES) - 4 and len(CPU_REF) >= 14


def valid(name, I):
    """finite floats, flags of 0 or 1, triangle indices inside the vertices"""
    for key, a in I.items():
        for field in (a.dtype.names or (None,)):
            x = a[field] if field else a
            if x.dtype.kind == "f":
                assert np.isfinite(x).all(), (name, key, field)
        if key == "keep":
            assert np.isin(a, (0, 1)).all(), name
        if key == "triangles":
            assert a.min() >= 0 and a.max() < (len(I["vertices"]) if "vertices" in I else SC.NV), name
        if key == "weight":
            assert (a >= 0).all(), name


@pytest.mark.parametrize("name", CPU_INPUTS)
def test_poison_is_valid_input_of_the_same_shape(name):
    case = SC.CASES[name]
    real = case.make("real")
    for kind in ("poison", "other"):
        I = case.make(kind)
        assert sorted(I) == sorted(real)
        for key in real:
            a, b = real[key], I[key]
            assert (a.dtype, a.shape, a.strides) == (b.dtype, b.shape, b.strides), (name, kind, key)
        valid(name, I)
        assert any(I[key].tobytes() != real[key].tobytes() for key in real), (name, kind)
    valid(name, real)


@pytest.mark.parametrize("name", CPU_REF)
def test_poison_changes_the_reference_answer(name):
    case = SC.CASES[name]
    want, _, host = case.ref(case.make("real"))
    assert sorted(want) == sorted(case.outs)
    for key, a in want.items():
        assert 0 < SC.as_bytes(a).size <= case.outs[key], (name, key)
    for kind in ("poison", "other"):
        got, _, ghost = case.ref(case.make(kind))
        assert any(SC.as_bytes(got[k]).tobytes() != SC.as_bytes(want[k]).tobytes() for k in want) or ghost != host, \
            (name, kind)
