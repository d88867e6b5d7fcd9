"""urdf.load_urdf_visuals on the host: the meshes of tests/drawer_scene_fixtures against vertices transformed by hand in float64, the
rules for several visuals, the collision fallback and `package://`, and the ValueErrors.  No GPU."""
import os

import numpy as np
import pytest

from tests import drawer_scene_fixtures as DS
from tests import mesh_bake_ref as MB


def _close(got, want64):
    """float32 `got` against float64 `want64` to fp32 rounding: one rounding of the result (2^-24 relative), with an absolute floor
    for coordinates a rotation takes to (nearly) zero."""
    assert got.dtype == np.float32
    np.testing.assert_allclose(got.astype(np.float64), want64, rtol=2.0 ** -23, atol=1e-9)


@pytest.mark.parametrize("kind", DS.KINDS)
def test_visuals_equal_the_vertices_transformed_by_hand(tmp_path, kind):
    from partmanip_amd.urdf import load_urdf, load_urdf_visuals
    folder = DS.write_cabinet(tmp_path, kind)
    path = os.path.join(folder, "mobility_new.urdf")
    tree = load_urdf(path, scale=DS.SCALE)
    got = load_urdf_visuals(path, scale=DS.SCALE)
    assert len(got) == tree.num_bodies
    seen = 0
    for name, entry in zip(tree.names, got):                  # the tree's body order
        want = DS.expected_visual(kind, name)
        if want is None:
            assert entry is None, name
            continue
        seen += 1
        v, f = entry
        _close(v, want[0])
        assert f.dtype == np.int64 and np.array_equal(f, want[1])
    assert seen == len(DS.SPEC[kind])
    assert [e is not None for e in got] == list(tree.has_mesh)            # load_urdf's own flag is unchanged and agrees


def test_the_origin_and_the_mesh_scale_are_not_trivial_in_the_fixture():
    v, _ = DS.expected_visual("A", "drawer", scale=1.0)
    plain = DS.SPEC["A"]["drawer"][0][0].astype(np.float64)
    assert np.abs(v - plain).max() > 0.05


def _write(tmp_path, body, meshes):
    from partmanip_amd import meshio
    for name, (v, f) in meshes.items():
        os.makedirs(os.path.dirname(os.path.join(tmp_path, name)), exist_ok=True)
        meshio.save_obj(os.path.join(tmp_path, name), v, f)
    path = os.path.join(tmp_path, "robot.urdf")
    with open(path, "w") as f:
        f.write(f'<robot name="r"><link name="root">{body}</link><link name="tip"/>'
                '<joint name="j" type="revolute"><parent link="root"/><child link="tip"/><axis xyz="0 0 1"/></joint></robot>')
    return path


def test_several_visuals_concatenate_and_collision_is_the_fallback(tmp_path):
    from partmanip_amd.urdf import load_urdf_visuals
    a, b = MB.box_mesh((0.1, 0.2, 0.3), (0, 0, 0)), MB.box_mesh((0.05, 0.05, 0.05), (1, 0, 0))
    body = ('<visual><geometry><mesh filename="package://m/a.obj"/></geometry></visual>'
            '<visual><geometry><box size="1 1 1"/></geometry></visual>'
            '<visual><origin xyz="0 0 2"/><geometry><mesh filename="m/b.obj" scale="2 2 2"/></geometry></visual>'
            '<collision><geometry><mesh filename="m/never.obj"/></geometry></collision>')
    root, tip = load_urdf_visuals(_write(tmp_path, body, {"m/a.obj": a, "m/b.obj": b}))
    assert tip is None
    v, f = root
    _close(v[:8], a[0].astype(np.float64))
    _close(v[8:], b[0].astype(np.float64) * 2 + np.array([0, 0, 2.0]))
    assert np.array_equal(f, np.concatenate([a[1], b[1] + 8]))
    # no visual with a mesh: the collision meshes
    body = ('<visual><geometry><box size="1 1 1"/></geometry></visual>'
            '<collision><origin xyz="1 0 0" rpy="0 0 1.5707963267948966"/><geometry><mesh filename="m/a.obj"/></geometry></collision>')
    (v, f), _ = load_urdf_visuals(_write(tmp_path, body, {}), scale=3.0)
    x = a[0].astype(np.float64)
    _close(v, (np.stack([-x[:, 1], x[:, 0], x[:, 2]], axis=1) + np.array([1.0, 0, 0])) * 3.0)      # a quarter turn about z
    assert np.array_equal(f, a[1])


def test_value_errors_name_the_file_and_the_link(tmp_path):
    from partmanip_amd.urdf import load_urdf_visuals
    with pytest.raises(ValueError, match=r"gone\.obj.*'root'"):
        load_urdf_visuals(_write(tmp_path, '<visual><geometry><mesh filename="m/gone.obj"/></geometry></visual>', {}))
    os.makedirs(os.path.join(tmp_path, "m"), exist_ok=True)
    with open(os.path.join(tmp_path, "m", "bad.obj"), "w") as f:
        f.write("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 4\n")
    with pytest.raises(ValueError, match=r"bad\.obj.*'root'"):
        load_urdf_visuals(_write(tmp_path, '<visual><geometry><mesh filename="m/bad.obj"/></geometry></visual>', {}))
    with open(os.path.join(tmp_path, "m", "mesh.ply"), "w") as f:
        f.write("ply\n")
    with pytest.raises(ValueError, match=r"mesh\.ply.*'root'"):
        load_urdf_visuals(_write(tmp_path, '<visual><geometry><mesh filename="m/mesh.ply"/></geometry></visual>', {}))
    with pytest.raises(ValueError, match="scale"):
        load_urdf_visuals(_write(tmp_path, "", {}), scale=0.0)


def test_load_drawer_meshes_reads_every_folder_at_the_assets_scale(tmp_path):
    assets, groups = DS.load_groups(tmp_path)
    assert [len(g) for g in groups] == [2, 7, 2] == [int(n) for n in assets.num_bodies]
    assert [sum(len(m[1]) for m in g if m is not None) for g in groups] == [24, 84, 300]
    assert groups[2][0] is None
    for kind, tree, bodies in zip(DS.KINDS, assets.trees, groups):
        for name, entry in zip(tree.names, bodies):
            want = DS.expected_visual(kind, name, scale=assets.scale)
            assert (entry is None) == (want is None)
            if entry is not None:
                _close(entry[0], want[0])
