"""Legacy VTK polygon meshes without vtk or ITK: ``itk.meshread`` / ``itk.meshwrite`` for ``DATASET POLYDATA`` files.

Read: ASCII and BINARY (big-endian, as the legacy format defines it); ``POINTS`` of any numeric type; ``POLYGONS`` in the count-prefixed
layout and in the 5.1 ``OFFSETS`` / ``CONNECTIVITY`` layout, every polygon with the same number of corners; ``POINT_DATA`` arrays given as
``SCALARS`` (with or without ``LOOKUP_TABLE``), ``VECTORS`` / ``NORMALS`` or ``FIELD``; ``CELL_DATA`` and ``METADATA`` are skipped.
Another dataset type, vertex / line / strip cells and mixed polygon sizes raise ``ValueError``.

Write: ``POINTS`` (float for float32 vertices, double for float64), ``POLYGONS`` (count-prefixed), each point array as ``SCALARS``
(1-4 components) or a ``FIELD`` array, ASCII by default or BINARY.  A float32 mesh with its point arrays round-trips bit for bit.
Host code only.
"""
from __future__ import annotations

import numpy as np

from .mesh_processing import Mesh

_TYPES = {"bit": None, "unsigned_char": "u1", "char": "i1", "unsigned_short": "u2", "short": "i2", "unsigned_int": "u4", "int": "i4",
          "unsigned_long": "u8", "long": "i8", "float": "f4", "double": "f8", "vtktypeint8": "i1", "vtktypeuint8": "u1",
          "vtktypeint16": "i2", "vtktypeuint16": "u2", "vtktypeint32": "i4", "vtktypeuint32": "u4", "vtktypeint64": "i8",
          "vtktypeuint64": "u8", "vtktypefloat32": "f4", "vtktypefloat64": "f8", "vtkidtype": "i8"}
_NAMES = {np.dtype("u1"): "unsigned_char", np.dtype("i1"): "char", np.dtype("u2"): "unsigned_short", np.dtype("i2"): "short",
          np.dtype("u4"): "unsigned_int", np.dtype("i4"): "int", np.dtype("u8"): "vtktypeuint64", np.dtype("i8"): "vtktypeint64",
          np.dtype("f4"): "float", np.dtype("f8"): "double"}


def _dtype(name: str) -> np.dtype:
    t = _TYPES.get(name.lower())
    if t is None:
        raise ValueError(f"unsupported VTK data type {name!r}")
    return np.dtype(t)


class _Reader:
    def __init__(self, data: bytes, binary: bool):
        self.b, self.pos, self.binary = data, 0, binary

    def line(self, allow_eof: bool = False):
        """The next non-blank line, stripped; None at the end of the file when ``allow_eof``."""
        while True:
            if self.pos >= len(self.b):
                if allow_eof:
                    return None
                raise ValueError("unexpected end of the VTK file")
            end = self.b.find(b"\n", self.pos)
            end = len(self.b) if end < 0 else end
            s = self.b[self.pos:end].decode("latin-1").strip()
            self.pos = end + 1
            if s:
                return s

    def peek(self):
        pos = self.pos
        try:
            return self.line(allow_eof=True)
        finally:
            self.pos = pos

    def values(self, count: int, dtype: np.dtype) -> np.ndarray:
        if count == 0:
            return np.zeros(0, dtype)
        if self.binary:
            nbytes = count * dtype.itemsize
            if self.pos + nbytes > len(self.b):
                raise ValueError("unexpected end of the VTK file in binary data")
            out = np.frombuffer(self.b, dtype.newbyteorder(">"), count, self.pos).astype(dtype)
            self.pos += nbytes
            return out
        tokens = []
        while len(tokens) < count:
            tokens.extend(self.line().split())
        if len(tokens) != count:
            raise ValueError(f"expected {count} values, the data lines hold {len(tokens)}")
        if dtype.kind == "f":
            return np.array([float(t) for t in tokens], np.float64).astype(dtype)
        return np.array([int(t) for t in tokens], np.int64).astype(dtype)

    def skip_metadata(self):
        if (self.peek() or "").upper().startswith("METADATA"):
            self.line()
            while self.pos < len(self.b):                   # the block ends at an empty line
                end = self.b.find(b"\n", self.pos)
                end = len(self.b) if end < 0 else end
                s = self.b[self.pos:end].strip()
                self.pos = end + 1
                if not s:
                    break


def _read_cells(r: _Reader, a: int, b: int):
    """(counts, connectivity) of a cell section whose header gave the numbers a, b: the count-prefixed layout (a cells, b ints) or
    the 5.1 layout (a offsets = cells + 1, b connectivity entries)."""
    head = r.peek()
    if head is not None and head.upper().startswith("OFFSETS"):
        off = r.values(a, _dtype(r.line().split()[1])).astype(np.int64)
        kw = r.line().split()
        if kw[0].upper() != "CONNECTIVITY":
            raise ValueError(f"expected CONNECTIVITY after OFFSETS, got {kw[0]!r}")
        conn = r.values(b, _dtype(kw[1])).astype(np.int64)
        if len(off) == 0:
            return np.zeros(0, np.int64), conn
        if off[0] != 0 or off[-1] != len(conn) or np.any(np.diff(off) < 0):
            raise ValueError("malformed OFFSETS")
        return np.diff(off), conn
    flat = r.values(b, np.dtype("i4")).astype(np.int64)
    counts, conn, i = np.zeros(a, np.int64), [], 0
    if a:
        # every cell of a triangle / quad mesh has the same size: check that fast, walk the list otherwise
        k = int(flat[0])
        if k > 0 and b == a * (k + 1) and np.all(flat[::k + 1] == k):
            return np.full(a, k, np.int64), flat.reshape(a, k + 1)[:, 1:].reshape(-1)
        for c in range(a):
            if i >= len(flat):
                raise ValueError("the cell list is shorter than its header says")
            counts[c] = flat[i]
            conn.append(flat[i + 1:i + 1 + flat[i]])
            i += 1 + int(flat[i])
        if i != b:
            raise ValueError("the cell list is longer than its counts")
    return counts, (np.concatenate(conn) if conn else np.zeros(0, np.int64))


def _read_attributes(r: _Reader, n: int, keep: bool, out: dict):
    """The arrays of one POINT_DATA / CELL_DATA section until the next section keyword."""
    while True:
        head = r.peek()
        if head is None:
            return
        kw = head.split()
        key = kw[0].upper()
        if key == "SCALARS":
            r.line()
            ncomp = int(kw[3]) if len(kw) > 3 else 1
            dt = _dtype(kw[2])
            nxt = r.peek()
            if nxt is not None and nxt.upper().startswith("LOOKUP_TABLE"):
                r.line()
            a = r.values(n * ncomp, dt)
            if keep:
                out[kw[1]] = a if ncomp == 1 else a.reshape(n, ncomp)
        elif key in ("VECTORS", "NORMALS"):
            r.line()
            a = r.values(3 * n, _dtype(kw[2])).reshape(n, 3)
            if keep:
                out[kw[1]] = a
        elif key == "TEXTURE_COORDINATES":
            r.line()
            a = r.values(int(kw[2]) * n, _dtype(kw[3])).reshape(n, int(kw[2]))
            if keep:
                out[kw[1]] = a
        elif key == "TENSORS":
            r.line()
            a = r.values(9 * n, _dtype(kw[2])).reshape(n, 3, 3)
            if keep:
                out[kw[1]] = a
        elif key == "COLOR_SCALARS":
            r.line()
            a = r.values(int(kw[2]) * n, np.dtype("u1") if r.binary else np.dtype("f4"))
            if keep:
                out[kw[1]] = a.reshape(n, int(kw[2]))
        elif key == "LOOKUP_TABLE":
            r.line()
            r.values(4 * int(kw[2]), np.dtype("u1") if r.binary else np.dtype("f4"))
        elif key == "FIELD":
            r.line()
            for _ in range(int(kw[2])):
                spec = r.line().split()
                if spec[0] == "NULL_ARRAY":
                    continue
                name, ncomp, ntup = spec[0], int(spec[1]), int(spec[2])
                a = r.values(ncomp * ntup, _dtype(spec[3]))
                r.skip_metadata()
                if keep:
                    out[name] = a if ncomp == 1 else a.reshape(ntup, ncomp)
        elif key == "METADATA":
            r.skip_metadata()
            continue
        else:
            return
        r.skip_metadata()


def read_vtk(path) -> Mesh:
    """A legacy VTK POLYDATA file as a ``Mesh`` (verts in the file's precision, faces int32 [m,k], point arrays)."""
    with open(path, "rb") as fh:
        data = fh.read()
    r = _Reader(data, False)
    first = r.line()
    if not first.startswith("# vtk DataFile"):
        raise ValueError(f"{path}: not a legacy VTK file")
    end = data.find(b"\n", r.pos)                      # the title line may be empty
    r.pos = len(data) if end < 0 else end + 1
    fmt = r.line().upper()
    if fmt not in ("ASCII", "BINARY"):
        raise ValueError(f"{path}: format {fmt!r} is neither ASCII nor BINARY")
    r.binary = fmt == "BINARY"
    ds = r.line().split()
    if len(ds) < 2 or ds[0].upper() != "DATASET" or ds[1].upper() != "POLYDATA":
        raise ValueError(f"{path}: only DATASET POLYDATA is supported, got {' '.join(ds)!r}")
    verts, faces, point_data = None, None, {}
    while True:
        head = r.peek()
        if head is None:
            break
        kw = head.split()
        key = kw[0].upper()
        if key == "METADATA":
            r.skip_metadata()
            continue
        if key == "FIELD":                                 # dataset-level field data: skipped
            _read_attributes(r, 0, False, {})
            continue
        r.line()
        if key == "POINTS":
            n = int(kw[1])
            verts = r.values(3 * n, _dtype(kw[2])).reshape(n, 3)
            r.skip_metadata()
        elif key in ("VERTICES", "LINES", "TRIANGLE_STRIPS", "POLYGONS"):
            counts, conn = _read_cells(r, int(kw[1]), int(kw[2]))
            r.skip_metadata()
            if key != "POLYGONS":
                if len(counts):
                    raise ValueError(f"{path}: {key.lower()} cells are not supported (only polygons)")
                continue
            if len(counts) and np.any(counts != counts[0]):
                raise ValueError(f"{path}: polygons of mixed sizes {sorted(set(counts.tolist()))} are not supported")
            k = int(counts[0]) if len(counts) else 3
            if k < 3:
                raise ValueError(f"{path}: polygons with {k} corners")
            faces = conn.reshape(len(counts), k)
        elif key == "POINT_DATA":
            _read_attributes(r, int(kw[1]), True, point_data)
        elif key == "CELL_DATA":
            _read_attributes(r, int(kw[1]), False, {})
        else:
            raise ValueError(f"{path}: unsupported section {kw[0]!r}")
    if verts is None:
        raise ValueError(f"{path}: no POINTS")
    if faces is None:
        faces = np.zeros((0, 3), np.int64)
    if faces.size and (faces.min() < 0 or faces.max() >= len(verts)):
        raise ValueError(f"{path}: a polygon indexes outside the {len(verts)} points")
    for name, a in point_data.items():
        if len(a) != len(verts):
            raise ValueError(f"{path}: point array {name!r} has {len(a)} tuples, the mesh has {len(verts)} points")
    return Mesh(verts, faces.astype(np.int32), point_data)


def _ascii(a: np.ndarray, per_line: int) -> bytes:
    flat = a.reshape(-1)
    if flat.dtype == np.float32:
        txt = np.char.mod("%.9g", flat.astype(np.float64))
    elif flat.dtype == np.float64:
        txt = np.char.mod("%.17g", flat)
    else:
        txt = flat.astype(str)
    rows = [" ".join(txt[i:i + per_line]) for i in range(0, len(txt), per_line)]
    return ("\n".join(rows) + "\n").encode() if rows else b""


def _data(a: np.ndarray, binary: bool, per_line: int = 9) -> bytes:
    if binary:
        return a.astype(a.dtype.newbyteorder(">")).tobytes() + b"\n"
    return _ascii(a, per_line)


def _array(a) -> np.ndarray:
    a = np.asarray(a)
    if a.dtype == np.bool_:
        a = a.astype(np.uint8)
    if a.dtype.newbyteorder("=") not in _NAMES:
        raise ValueError(f"point array of dtype {a.dtype} cannot be written to VTK")
    return np.ascontiguousarray(a, a.dtype.newbyteorder("="))


def write_vtk(mesh: Mesh, path, binary: bool = False, title: str = "oai_analysis_2_amd mesh") -> None:
    """``mesh`` as a legacy VTK POLYDATA file (version 3.0 layout, readable by VTK, ITK and ParaView)."""
    verts = np.asarray(mesh.verts)
    if verts.dtype not in (np.float32, np.float64):
        verts = verts.astype(np.float32)
    verts = np.ascontiguousarray(verts).reshape(-1, 3)
    faces = np.asarray(mesh.faces)
    faces = faces.reshape(len(faces), -1) if faces.size else np.zeros((0, 3), np.int64)
    n, m, k = len(verts), len(faces), faces.shape[1]
    if m and (faces.min() < 0 or faces.max() >= n):
        raise ValueError("write_vtk: a face indexes outside the mesh's points")
    out = [b"# vtk DataFile Version 3.0\n", title.replace("\n", " ")[:255].encode() + b"\n", b"BINARY\n" if binary else b"ASCII\n",
           b"DATASET POLYDATA\n", f"POINTS {n} {_NAMES[verts.dtype]}\n".encode(), _data(verts, binary)]
    if m:
        cells = np.empty((m, k + 1), np.int32)
        cells[:, 0] = k
        cells[:, 1:] = faces
        out += [f"POLYGONS {m} {m * (k + 1)}\n".encode(), _data(cells, binary, k + 1)]
    arrays = [(name, _array(a)) for name, a in mesh.point_data.items()]
    if arrays:
        out.append(f"POINT_DATA {n}\n".encode())
    for name, a in arrays:
        if " " in name or not name:
            raise ValueError(f"write_vtk: array name {name!r} must be non-empty and hold no space")
        if len(a) != n:
            raise ValueError(f"write_vtk: point array {name!r} has {len(a)} tuples, the mesh has {n} points")
        ncomp = int(np.prod(a.shape[1:], dtype=np.int64))
        if a.ndim <= 2 and 1 <= ncomp <= 4:
            out += [f"SCALARS {name} {_NAMES[a.dtype]} {ncomp}\nLOOKUP_TABLE default\n".encode(), _data(a, binary, max(ncomp, 9))]
        else:
            out += [f"FIELD FieldData 1\n{name} {ncomp} {n} {_NAMES[a.dtype]}\n".encode(), _data(a, binary, ncomp)]
    with open(path, "wb") as fh:
        fh.write(b"".join(out))
