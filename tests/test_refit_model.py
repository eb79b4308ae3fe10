"""CPU: the numpy model of include/pt_refit.h (tests/_refit_model.py), which tests/test_gpu_refit.py holds the device to, held to facts that need no
GPU: on a scene's own triangles it gives back the scene's own boxes bit for bit, on a scaled scene the rebuilt boxes and four times the cost, and
the hand cases of the header's rule."""
import numpy as np
import pytest

import _refit_cases as RC
import _refit_model as RM

f32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def _identity(b):
    out, cost = RM.refit_buffers(b)
    assert np.array_equal(_bits(out), _bits(b[10]))
    assert len(cost) == int(b[13][0]) and np.isfinite(cost).all() and (cost >= 0).all()
    return cost


@pytest.mark.parametrize("name", list(RC.WORKLOADS))
def test_identity_on_the_workloads(pt, name):
    b = RC.workloads(pt)[name]
    assert int(b[13][0]) >= 1 and len(b[11]) // 3 >= 3
    if name == "C6":
        assert int(b[13][0]) == 64
    _identity(b)


@pytest.mark.parametrize("name", [f"soup{n}" for n, _, _ in RC.SOUPS] + ["ladder", "loose"])
def test_identity_on_the_extra_inputs(pt, name):
    b = RC.extra(pt)[name]
    cost = _identity(b)
    _, height, order = RM.structure(b[10], b[11], b[13])
    if name == "ladder":
        assert len(b[3]) // 40 == 330 and height.max() == 180             # the reference's builder gives up at depth 180 here (a leaf of 150)
    if name == "loose":
        used = set(int(t) for t in b[12])
        assert len(b[3]) // 40 == 60 and len(used) == 57 and not {0, 41, 59} & used and len(cost) == 2
    if name.startswith("soup"):
        assert len(cost) == 2 and len(order) == len(b[11]) // 3


def test_hand_made_chain_has_256_heights_and_a_refit_is_a_fixed_point(pt):
    """the builder's ladder stops at 180 heights, so the deepest tree the reference's depth limit allows is made by hand; its stale boxes are no
    identity case, but a second refit of the first one's result changes nothing"""
    b = RC.extra(pt)["chain256"]
    _, height, order = RM.structure(b[10], b[11], b[13])
    assert height.max() == 256 and len(order) == 513 and sorted(height.tolist()) == sorted([0] * 257 + list(range(1, 257)))
    out, cost = RM.refit_buffers(b)
    again, cost2 = RM.refit(out, b[11], b[12], b[13], b[3])
    assert np.array_equal(_bits(out), _bits(again)) and np.array_equal(cost, cost2) and cost[0] > 0
    v = RM.vertices(b[3]).reshape(-1, 3)
    assert np.array_equal(out[0:3], v.min(axis=0)) and np.array_equal(out[3:6], v.max(axis=0))


def test_scaled_scene_has_the_same_topology_the_rebuilt_boxes_and_four_times_the_cost(pt):
    """scale=(2, 2, 2), the second object's shift doubled with it: scaling by 2 is exact in binary32 and binary64 and commutes with rounding, so the
    builder's comparisons come out the same: the precondition, asserted first"""
    for n, d, s in ((65, 0.0, 3), (64, 0.5, 4), (1000, 0.0, 5)):
        one, two = RC.soup(pt, n, d, s), RC.soup(pt, n, d, s, scale=2.0)
        for k in (11, 12, 13):
            assert np.array_equal(one[k], two[k]), k
        assert not np.array_equal(_bits(one[10]), _bits(two[10]))
        out, cost = RM.refit(one[10], one[11], one[12], one[13], two[3])
        assert np.array_equal(_bits(out), _bits(two[10]))
        _, cost1 = RM.refit_buffers(one)
        assert (cost1 > 0).all() and np.array_equal(cost, 4.0 * cost1)


def _tri(*verts):
    t = np.zeros(40, f32)
    for k, v in enumerate(verts):
        t[4 * k:4 * k + 3] = v
    return t


def _hand_tree():
    """node 0 = (1, 4); 1 = (2, 3); leaves 2: triangle 0, 3: empty, 4: triangles 1 and 2; node 5: a leaf no root reaches"""
    tree = np.array([0, 1, 4, 1, 2, 3, 2, -1, -1, 3, -1, -1, 4, -1, -1, 5, -1, -1], np.int32)
    data = np.zeros((6, 8), f32)
    data[:, 0:6] = 77.0                                           # stale boxes
    data[3, 0:6] = (-9, -8, -7, -6, -5, -4)                       # the empty leaf's box
    data[5] = (1, 2, 3, 4, 5, 6, 0, 3)                            # unreachable: copied whole
    data[2, 6:8], data[3, 6:8], data[4, 6:8] = (0, 1), (1, 1), (1, 3)
    data[0, 6:8] = (123, 456)                                     # floats 6 and 7 are copied even where nothing reads them
    leaf = np.array([0, 2, 1], np.int32)
    roots = np.array([1, 0], np.int32)
    return data.reshape(-1), tree, leaf, roots


def test_hand_cases_signed_zero_empty_leaf_and_unreachable_node():
    data, tree, leaf, roots = _hand_tree()
    tris = np.concatenate([_tri((0.0, 1, 2), (-0.0, 1, 3), (0.0, 2, 2)),          # x: +0, -0, +0 -> min -0.0, max +0.0
                           _tri((1, 1, 1), (2, 1, 1), (1, 2, 1)), _tri((3, 0, -0.0), (3, 1, -0.0), (4, 0, -0.0))])
    out, cost = RM.refit(data, tree, leaf, roots, tris)
    out = out.reshape(6, 8)
    assert _bits(out[2, 0:6]).tolist() == _bits(np.array([-0.0, 1, 2, 0.0, 2, 3], f32)).tolist()
    assert _bits(out[4, 0:6]).tolist() == _bits(np.array([1, 0, -0.0, 4, 2, 1], f32)).tolist()
    assert np.array_equal(_bits(out[3]), _bits(data.reshape(6, 8)[3]))                     # the empty leaf keeps its box
    assert _bits(out[1, 0:6]).tolist() == _bits(np.array([-9, -8, -7, 0.0, 2, 3], f32)).tolist()      # ... and takes part in its parent's union
    assert _bits(out[0, 0:6]).tolist() == _bits(np.array([-9, -8, -7, 4, 2, 3], f32)).tolist()
    assert np.array_equal(_bits(out[5]), _bits(data.reshape(6, 8)[5]))                     # unreachable: untouched
    assert np.array_equal(_bits(out[:, 6:8]), _bits(data.reshape(6, 8)[:, 6:8]))
    # cost by hand: leaf 2 has s = (0, 1, 1): A = 1, one triangle; leaf 3 counts 0 triangles; leaf 4 has s = (3, 2, 1): A = 11, two triangles
    A1 = (9.0 * 10.0 + 9.0 * 10.0) + 10.0 * 10.0
    A0 = (13.0 * 10.0 + 13.0 * 10.0) + 10.0 * 10.0
    assert cost.tolist() == [A0 + ((A1 + (1.0 + 0.0)) + 22.0)]
    # a zero of either sign beside a non-zero value, and the union of a -0.0 box with a +0.0 box
    assert _bits(RM.unkey(np.minimum(RM.key(f32(-0.0)), RM.key(f32(0.0))))) == 0x80000000
    assert _bits(RM.unkey(np.maximum(RM.key(f32(-0.0)), RM.key(f32(0.0))))) == 0
    x = np.array([-np.inf, -1.5, -1e-45, -0.0, 0.0, 1e-45, 2.5, np.inf], f32)
    assert (np.diff(RM.key(x).astype(np.int64)) > 0).all() and np.array_equal(_bits(RM.unkey(RM.key(x))), _bits(x))


def test_nan_in_a_referenced_triangle_is_refused_and_elsewhere_is_not():
    data, tree, leaf, roots = _hand_tree()
    tris = np.concatenate([_tri((0, 1, 2), (0, 1, 3), (0, 2, 2)), _tri((1, 1, 1), (2, 1, 1), (1, 2, 1)), _tri((3, 0, 0), (3, 1, 0), (4, 0, 0)),
                           _tri((np.nan, 0, 0), (0, 0, 0), (0, 0, 0))])          # triangle 3: referenced by nothing
    assert RM.refit(data, tree, leaf, roots, tris) is not None
    bad = tris.copy(); bad[40 + 9] = np.nan                                       # float 9 of triangle 1: its third vertex's y
    assert RM.refit(data, tree, leaf, roots, bad) is None
    ok = tris.copy(); ok[40 + 3] = np.nan; ok[40 + 11:40 + 40] = np.nan           # the floats of the record that are no vertex
    assert RM.refit(data, tree, leaf, roots, ok) is not None
    inf = tris.copy(); inf[0] = np.inf
    assert RM.refit(data, tree, leaf, roots, inf)[0].reshape(6, 8)[0, 3] == np.inf
