"""CPU: the cuberille contract through its numpy restatement (tests/cuberille_ref.py) on hand cases and random blobs, the argument
checks of oai_cuberille_* (every one returns an error before any GPU work), and the legacy VTK reader / writer (io_vtk)."""
import ctypes as C
import inspect
from collections import Counter

import numpy as np
import pytest

import cuberille_ref as ref
from oai_analysis_2_amd import _lib, meshread, meshwrite
from oai_analysis_2_amd.mesh_processing import Mesh


def _vol(shape, inside):
    v = np.zeros(shape, np.float32)
    for z, y, x in inside:
        v[z, y, x] = 1.0
    return v


def _edges(tris):
    return np.concatenate([tris[:, [0, 1]], tris[:, [1, 2]], tris[:, [2, 0]]])


def _closed_and_oriented(tris):
    e = [tuple(x) for x in _edges(tris)]
    return Counter(e) == Counter((b, a) for a, b in e)


# ---- hand cases --------------------------------------------------------------------------------------------------------------
def test_one_voxel():
    r = ref.cuberille(_vol((3, 3, 3), [(1, 1, 1)]), project_vertices=False)
    assert len(r["verts"]) == 8 and len(r["faces"]) == 12
    assert _closed_and_oriented(r["faces"])
    assert ref.signed_volume6(r["verts64"], r["faces"], center=False) == 6.0
    # the corners of the voxel at index (1,1,1): continuous index 0.5 .. 1.5
    assert sorted(map(tuple, r["verts"].tolist())) == [(x, y, z) for x in (0.5, 1.5) for y in (0.5, 1.5) for z in (0.5, 1.5)]
    # face order -z -y -x +x +y +z: the first quad lies in z = 0.5, the last in z = 1.5, the fourth in x = 1.5
    q = r["quads"]
    assert np.all(r["verts"][q[0], 2] == 0.5) and np.all(r["verts"][q[5], 2] == 1.5) and np.all(r["verts"][q[3], 0] == 1.5)
    # vertices in order of first use: the first quad's corners are vertices 0..3
    assert q[0].tolist() == [0, 1, 2, 3]


def test_two_face_adjacent_voxels():
    r = ref.cuberille(_vol((2, 3, 4), [(1, 1, 1), (1, 1, 2)]), project_vertices=False)
    assert len(r["verts"]) == 12 and len(r["faces"]) == 20
    assert _closed_and_oriented(r["faces"])
    assert ref.signed_volume6(r["verts64"], r["faces"], center=False) == 12.0


def test_edge_contact_is_a_non_manifold_edge():
    """Two voxels that share only an edge share its 2 lattice points; the vertices are not split, so that edge bounds 4 triangles."""
    r = ref.cuberille(_vol((1, 2, 2), [(0, 0, 0), (0, 1, 1)]), project_vertices=False)
    assert len(r["verts"]) == 14 and len(r["faces"]) == 24
    lat = r["lattice"]
    shared = [i for i, p in enumerate(lat.tolist()) if p[0] == 1 and p[1] == 1]
    assert len(shared) == 2
    und = Counter(tuple(sorted(e)) for e in _edges(r["faces"]).tolist())
    assert und[tuple(sorted(shared))] == 4
    assert _closed_and_oriented(r["faces"])
    assert ref.signed_volume6(r["verts64"], r["faces"], center=False) == 12.0


def test_border_voxel_is_closed():
    v = np.zeros((2, 2, 2), np.float32)
    v[0, 0, 0] = 0.9
    r = ref.cuberille(v, project_vertices=False)
    assert len(r["verts"]) == 8 and len(r["faces"]) == 12 and _closed_and_oriented(r["faces"])
    full = ref.cuberille(np.ones((2, 3, 4), np.float32), project_vertices=False)           # every face on the border
    assert len(full["faces"]) == 2 * 2 * (2 * 3 + 3 * 4 + 2 * 4) and _closed_and_oriented(full["faces"])
    assert ref.signed_volume6(full["verts64"], full["faces"], center=False) == 6.0 * 24


def test_iso_value_itself_is_inside():
    v = np.full((3, 3, 3), 0.25, np.float32)
    v[1, 1, 1] = np.float32(0.5)
    assert len(ref.cuberille(v, iso=0.5, project_vertices=False)["faces"]) == 12
    v[1, 1, 1] = np.nextafter(np.float32(0.5), np.float32(0))
    assert len(ref.cuberille(v, iso=0.5, project_vertices=False)["faces"]) == 0


def test_quads_and_winding_flip():
    v = _vol((3, 3, 3), [(1, 1, 1)])
    q = ref.cuberille(v, triangles=False, project_vertices=False)
    t = ref.cuberille(v, project_vertices=False)
    assert q["faces"].shape == (6, 4)
    assert np.array_equal(t["faces"][0::2], q["faces"][:, [0, 1, 2]]) and np.array_equal(t["faces"][1::2], q["faces"][:, [0, 2, 3]])
    refl = np.diag([1.0, -1.0, 1.0])
    tf = ref.cuberille(v, direction=refl, project_vertices=False)
    qf = ref.cuberille(v, direction=refl, triangles=False, project_vertices=False)
    assert np.array_equal(tf["quads"], t["quads"])                                 # the numbering does not change
    assert np.array_equal(tf["faces"][0::2], t["faces"][0::2][:, [0, 2, 1]]) and np.array_equal(qf["faces"], q["faces"][:, [0, 3, 2, 1]])
    assert ref.signed_volume6(tf["verts64"], tf["faces"], center=False) == 6.0


# ---- random blobs: closed, oriented, exact volume ---------------------------------------------------------------------------
def _blob(seed, shape=(9, 11, 10)):
    rng = np.random.default_rng(seed)
    v = rng.random(shape).astype(np.float32)
    for _ in range(2):                                            # a little smoothing: blobs with holes, handles and edge contacts
        v = (v + np.roll(v, 1, 0) + np.roll(v, 1, 1) + np.roll(v, 1, 2)) / np.float32(4)
    return v


def _rotation(seed):
    q, _ = np.linalg.qr(np.random.default_rng(seed).normal(size=(3, 3)))
    return q if np.linalg.det(q) > 0 else -q


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_random_blobs_closed_oriented_volume(seed):
    v = _blob(seed)
    iso = float(np.median(v))
    n_inside = int((v >= np.float32(iso)).sum())
    r = ref.cuberille(v, iso, project_vertices=False)
    assert len(r["faces"]) > 100 and _closed_and_oriented(r["faces"])
    assert ref.signed_volume6(r["verts64"], r["faces"], center=False) == 6.0 * n_inside
    sp, org = (0.36, 0.5, 0.7), (-12.5, 3.25, 40.0)
    for d in (_rotation(seed), _rotation(seed) @ np.diag([1.0, 1.0, -1.0])):
        g = ref.cuberille(v, iso, spacing=sp, origin=org, direction=d, project_vertices=False)
        assert np.array_equal(g["quads"], r["quads"]) and _closed_and_oriented(g["faces"])
        want = n_inside * abs(np.linalg.det(d @ np.diag(sp)))
        assert abs(ref.signed_volume6(g["verts64"], g["faces"]) / 6.0 - want) <= 1e-9 * want


def test_projection_restatement_reaches_the_analytic_surface():
    e = ref.ellipsoid_case((20, 22, 20))
    for move in (False, True):
        a = ref.cuberille(e["vol"], spacing=e["spacing"], move_after_converged=move)
        dist = e["distance"](a["verts64"])
        slack = 0.0 if not move else ref.last_step(a["steps"], 0.25 * max(e["spacing"]))
        assert np.all(dist <= 0.1 * max(e["spacing"]) + slack) and a["steps"].max() < 50


# ---- C ABI argument checks ---------------------------------------------------------------------------------------------------
def test_abi_argument_checks():
    lib = _lib.load()
    d = (C.c_double * 64)()
    err = lambda: lib.oai_last_error()
    nv, nf = C.c_longlong(), C.c_longlong()
    assert lib.oai_cuberille_workspace_bytes(0, 4, 4) == 0 and lib.oai_cuberille_workspace_bytes(4, -1, 4) == 0
    assert lib.oai_cuberille_workspace_bytes(2048, 2048, 2048) == 0                     # corner slots would overflow 32 bits
    wb = int(lib.oai_cuberille_workspace_bytes(4, 5, 6))
    assert wb > 4 * 5 * 6 * 9
    c = lambda **kw: lib.oai_cuberille_count(kw.get("vol", d), kw.get("D", 4), 5, 6, kw.get("iso", 0.5), kw.get("ws", d), kw.get("wb", wb),
                                             kw.get("pnv", C.byref(nv)), kw.get("pnf", C.byref(nf)), None)
    assert c(vol=None) != 0 and b"null" in err()
    assert c(ws=None) != 0 and b"null" in err()
    assert c(pnv=None) != 0 and b"null" in err()
    assert c(pnf=None) != 0 and b"null" in err()
    assert c(D=0) != 0 and b"at least 1" in err()
    assert c(D=1 << 24) != 0 and b"too large" in err()
    assert c(iso=float("nan")) != 0 and b"NaN" in err()
    assert c(wb=wb - 1) != 0 and b"workspace" in err()
    geo = (C.c_double * 24)(*([0.0] * 3 + [1.0] * 3 + [1, 0, 0, 0, 1, 0, 0, 0, 1] * 2))

    def e(**kw):
        g = kw.get("geo", geo)
        return lib.oai_cuberille_emit(kw.get("vol", d), kw.get("D", 4), 5, 6, 0.5, g, 0, 1, kw.get("project", 1), kw.get("thr", 0.05),
                                      kw.get("step", -1.0), kw.get("relax", 0.95), kw.get("max_steps", 50), 1, kw.get("ws", d), kw.get("wb", wb),
                                      kw.get("nv", 10), kw.get("nf", 10), kw.get("verts", d), kw.get("faces", d), None, None)
    assert e(vol=None) != 0 and b"null" in err()
    assert e(geo=None) != 0 and b"null" in err()
    assert e(ws=None) != 0 and b"null" in err()
    assert e(verts=None) != 0 and b"null" in err()
    assert e(faces=None) != 0 and b"null" in err()
    assert e(D=-3) != 0 and b"at least 1" in err()
    assert e(nv=-1) != 0 and b"negative" in err()
    assert e(wb=wb - 1) != 0 and b"workspace" in err()
    bad = (C.c_double * 24)(*geo)
    bad[4] = 0.0
    assert e(geo=bad) != 0 and b"spacing" in err()
    bad[4] = float("inf")
    assert e(geo=bad) != 0 and b"non-finite" in err()
    assert e(thr=-0.1) != 0 and b"threshold" in err()
    assert e(relax=0.0) != 0 and b"relaxation" in err()
    assert e(max_steps=-1) != 0 and b"max_steps" in err()
    assert e(step=float("nan")) != 0 and b"step length" in err()


def test_python_surface():
    from oai_analysis_2_amd import mesh_processing as mp
    sig = inspect.signature(mp.get_mesh_from_probability_map)
    defaults = {k: p.default for k, p in sig.parameters.items() if k != "image"}
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for k, p in sig.parameters.items() if k != "image")
    assert defaults["iso_surface_value"] == 0.5 and defaults["generate_triangle_faces"] is True
    assert defaults["project_vertices_to_iso_surface"] is True and defaults["project_vertex_surface_distance_threshold"] == 0.05
    assert defaults["project_vertex_step_length"] == -1.0 and defaults["project_vertex_step_length_relaxation_factor"] == 0.95
    assert defaults["project_vertex_maximum_number_of_steps"] == 50 and defaults["move_after_converged"] is True
    assert callable(mp.cuberille_device)


# ---- legacy VTK I/O ----------------------------------------------------------------------------------------------------------
def _mesh(seed=0, k=3, n=50, m=80):
    rng = np.random.default_rng(seed)
    verts = (rng.normal(size=(n, 3)) * 1e3).astype(np.float32)
    verts[0] = [np.float32(1e-38), np.float32(-0.0), np.float32(3.4e38)]
    verts[1] = np.nextafter(np.float32(1.0), np.float32(2.0))
    faces = rng.integers(0, n, size=(m, k)).astype(np.int32)
    return Mesh(verts, faces, {"Distance": rng.random(n).astype(np.float32), "normals": rng.normal(size=(n, 3)).astype(np.float32),
                               "label": rng.integers(-5, 5, n).astype(np.int32), "d64": rng.random(n)})


@pytest.mark.parametrize("binary", [False, True])
@pytest.mark.parametrize("k", [3, 4])
def test_vtk_round_trip(tmp_path, binary, k):
    m = _mesh(k=k)
    path = str(tmp_path / "m.vtk")
    meshwrite(m, path, binary=binary)
    got = meshread(path)
    assert got.verts.dtype == np.float32 and got.verts.tobytes() == m.verts.tobytes()
    assert got.faces.dtype == np.int32 and np.array_equal(got.faces, m.faces)
    assert set(got.point_data) == set(m.point_data)
    for name, a in m.point_data.items():
        assert got.point_data[name].dtype == a.dtype and got.point_data[name].tobytes() == a.tobytes(), name
    with open(path, "rb") as fh:
        head = fh.read(80)
    assert head.startswith(b"# vtk DataFile Version 3.0\n") and (b"BINARY" in head) == binary


def test_vtk_round_trip_of_a_cuberille_mesh(tmp_path):
    r = ref.cuberille(_blob(7), 0.5, spacing=(0.36, 0.36, 0.7), origin=(1.0, -2.0, 3.5))
    m = Mesh(r["verts"], r["faces"], {"steps": r["steps"]})
    for binary in (False, True):
        meshwrite(m, str(tmp_path / "c.vtk"), binary=binary)
        got = meshread(str(tmp_path / "c.vtk"))
        assert got.verts.tobytes() == m.verts.tobytes() and np.array_equal(got.faces, m.faces)
        assert np.array_equal(got.point_data["steps"], r["steps"])


ASCII_COUNTS = """# vtk DataFile Version 2.0
File written by itkPolyDataMeshIO
ASCII
DATASET POLYDATA
POINTS 4 double
0 0 0 1 0 0
0 1 0
0 0 1
POLYGONS 4 16
3 0 2 1
3 0 1 3
3 0 3 2
3 1 2 3
CELL_DATA 4
SCALARS cellid int 1
LOOKUP_TABLE default
0 1 2 3
POINT_DATA 4
SCALARS pointData float
LOOKUP_TABLE default
0.5 1.5 2.5 3.5
FIELD FieldData 2
thick 1 4 double
1 2 3 4
vec 2 4 float
1 2 3 4 5 6 7 8
METADATA
INFORMATION 0

"""

ASCII_51 = """# vtk DataFile Version 5.1
vtk output
ASCII
DATASET POLYDATA
POINTS 4 float
0 0 0 1 0 0 0 1 0
0 0 1
METADATA
INFORMATION 2
NAME L2_NORM_RANGE LOCATION vtkDataArray
DATA 2 0 1
NAME L2_NORM_FINITE_RANGE LOCATION vtkDataArray
DATA 2 0 1

POLYGONS 5 12
OFFSETS vtktypeint64
0 3 6 9 12
CONNECTIVITY vtktypeint64
0 2 1 0 1 3 0 3 2 1 2 3
POINT_DATA 4
FIELD FieldData 1
Distance 1 4 float
0.25 0.5 0.75 1
"""


def test_vtk_reads_hand_written_files(tmp_path):
    p = tmp_path / "a.vtk"
    p.write_text(ASCII_COUNTS)
    m = meshread(str(p))
    assert m.verts.dtype == np.float64 and m.verts.shape == (4, 3) and m.verts[3].tolist() == [0, 0, 1]
    assert m.faces.tolist() == [[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]]
    assert m.point_data["pointData"].tolist() == [0.5, 1.5, 2.5, 3.5] and m.point_data["pointData"].dtype == np.float32
    assert m.point_data["thick"].tolist() == [1, 2, 3, 4] and m.point_data["vec"].shape == (4, 2)
    assert "cellid" not in m.point_data
    p.write_text(ASCII_51)
    m51 = meshread(str(p))
    assert m51.verts.dtype == np.float32 and np.array_equal(m51.faces, m.faces)
    assert m51.point_data["Distance"].tolist() == [0.25, 0.5, 0.75, 1.0]
    # the same 5.1 file in BINARY: big-endian int64 offsets / connectivity, big-endian float points
    b = (b"# vtk DataFile Version 5.1\nvtk output\nBINARY\nDATASET POLYDATA\nPOINTS 4 float\n" + m51.verts.astype(">f4").tobytes()
         + b"\nPOLYGONS 5 12\nOFFSETS vtktypeint64\n" + np.array([0, 3, 6, 9, 12], ">i8").tobytes()
         + b"\nCONNECTIVITY vtktypeint64\n" + m51.faces.reshape(-1).astype(">i8").tobytes() + b"\n")
    p.write_bytes(b)
    mb = meshread(str(p))
    assert np.array_equal(mb.verts, m51.verts) and np.array_equal(mb.faces, m51.faces)
    # mixed-size polygons in the count-prefixed layout are walked, then refused
    p.write_text(ASCII_COUNTS.split("POLYGONS")[0] + "POLYGONS 2 9\n3 0 1 2\n4 0 1 2 3\n")
    with pytest.raises(ValueError, match="mixed"):
        meshread(str(p))


@pytest.mark.parametrize("text,match", [
    (ASCII_COUNTS.replace("DATASET POLYDATA", "DATASET UNSTRUCTURED_GRID"), "POLYDATA"),
    (ASCII_COUNTS.split("POLYGONS")[0] + "LINES 1 3\n2 0 1\n", "lines"),
    (ASCII_COUNTS.split("POLYGONS")[0] + "VERTICES 2 4\n1 0\n1 1\n", "vertices"),
    (ASCII_COUNTS.split("POLYGONS")[0] + "TRIANGLE_STRIPS 1 5\n4 0 1 2 3\n", "triangle_strips"),
    (ASCII_COUNTS.replace("ASCII", "XML"), "neither"),
    (ASCII_COUNTS.replace("3 1 2 3", "3 1 2 9"), "outside"),
])
def test_vtk_refuses_unsupported_files(tmp_path, text, match):
    p = tmp_path / "bad.vtk"
    p.write_text(text)
    with pytest.raises(ValueError, match=match):
        meshread(str(p))
