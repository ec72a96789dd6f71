"""Scenes and meshes on disk, host side: the one reader and writer of a saved scene (<scene>.npz), PLY in and out, the scene
list and a ScanNet-layout scene directory.  The tools import these; this module imports none of them.  A scene file has
one of three layouts:
    dense    tsdf / semantic / instance as [X,Y,Z] volumes (the reference's arrays, utils.py:360-366)
    sparse   voxel rows under distinct keys: sparse_coords int32[M,3] relative to `origin`, sparse_tsdf f32[M],
             sparse_semantic / sparse_instance int32[M], dims
    legacy   (round 3) rows under the DENSE key names next to `coords` and `dims`; read, never written
"""
import os
from types import SimpleNamespace

import numpy as np
import torch

VOLUME_KEYS = ("tsdf", "semantic", "instance")
LABEL_KEYS = VOLUME_KEYS[1:]               # what the label tools ask for: they never touch the TSDF
_DEFAULTS = {"tsdf": (1.0, np.float32), "semantic": (0, np.int32), "instance": (0, np.int32)}     # models/gru_fusion.py:232-252


def _stored_shape(z, key):
    """shape of an entry from its .npy header: the array itself is not decompressed"""
    with z.zip.open(key + ".npy") as fh:
        version = np.lib.format.read_magic(fh)
        return (np.lib.format.read_array_header_1_0 if version == (1, 0) else np.lib.format.read_array_header_2_0)(fh)[0]


def read_scene(path, want=VOLUME_KEYS, rest=False):
    """<scene>.npz -> a record: layout ("dense" / "sparse" / "legacy"), origin float32[3], voxel_size, dims, arrays (the `want`
    ones of VOLUME_KEYS as stored: [X,Y,Z] volumes when dense, else [M] rows at coords [M,3]) and rest (every other entry as
    stored, when asked for).  One open, closed again; an entry is decompressed at most once, an array nobody wants never.
    ValueError for a file of none of the layouts."""
    with np.load(path) as z:
        files = set(z.files)
        # THE layout rule (load_scene_npz's): rows under their own keys; else the earlier rows under the dense names, known
        # by a 1-D tsdf next to coords and dims; else three volumes
        if "sparse_coords" in files:
            layout = "sparse"
        elif {"coords", "dims", "tsdf"} <= files and len(_stored_shape(z, "tsdf")) == 1:
            layout = "legacy"
        elif set(VOLUME_KEYS) <= files and all(len(_stored_shape(z, k)) == 3 for k in VOLUME_KEYS):
            layout = "dense"
        else:
            raise ValueError(f"{path}: none of the dense, sparse and legacy layouts of a saved scene")
        pre = "sparse_" if layout == "sparse" else ""
        arrays = {k: z[pre + k] for k in want}
        coords = None if layout == "dense" else z[pre + "coords"]
        taken = {pre + k for k in VOLUME_KEYS + ("coords",)}
        head = {k: z[k] for k in (z.files if rest else ("origin", "voxel_size", "dims")) if k in files and k not in taken}
        dims = _stored_shape(z, "tsdf") if layout == "dense" else head["dims"]
    return SimpleNamespace(layout=layout, origin=np.asarray(head["origin"], np.float32).reshape(3), arrays=arrays, coords=coords,
                           voxel_size=float(np.asarray(head["voxel_size"], np.float64)), dims=tuple(int(d) for d in dims),
                           rest=head if rest else {})


def _upload(values, key, device):
    return torch.from_numpy(np.ascontiguousarray(values).astype(_DEFAULTS[key][1], copy=False)).to(device or "cpu")


def scatter_volumes(dims, coords, rows, device=None):
    """voxel rows -> dense volumes: {key: values[M]} at coords [M,3] -> {key: [X,Y,Z] tensor}, TSDF f32 default 1, ids int32
    default 0, built on `device` (None: the host) from one upload of the coordinates and one per array"""
    c = torch.from_numpy(np.ascontiguousarray(coords).astype(np.int64).reshape(-1, 3)).to(device or "cpu")
    out = {}
    for key, values in rows.items():
        values = _upload(values, key, device)
        out[key] = torch.full(tuple(int(d) for d in dims), _DEFAULTS[key][0], dtype=values.dtype, device=values.device)
        out[key][c[:, 0], c[:, 1], c[:, 2]] = values
    return out


def scene_volumes(path, device=None, want=VOLUME_KEYS):
    """<scene>.npz in any layout -> (the `want` volumes in that order: tsdf f32, semantic / instance int32 [X,Y,Z] on
    `device`, origin float32[3], voxel_size).  Rows become volumes on the device."""
    s = read_scene(path, want)
    dense = s.layout == "dense"
    vols = {k: _upload(v, k, device) for k, v in s.arrays.items()} if dense else scatter_volumes(s.dims, s.coords, s.arrays, device)
    return tuple(vols[k] for k in want) + (s.origin, s.voxel_size)


def raster_rows(scene):
    """Scene (all three arrays) -> (cells int64[M,3] in raster order, their tsdf, semantic, instance values as stored,
    order: the file position of every row, None for a dense file).  The rows of a dense file are its cells with tsdf != 1,
    semantic != 0 or instance != 0."""
    a = scene.arrays
    if scene.layout == "dense":
        cells = np.argwhere((a["tsdf"] != 1) | (a["semantic"] != 0) | (a["instance"] != 0))
        return (cells,) + tuple(a[k][cells[:, 0], cells[:, 1], cells[:, 2]] for k in VOLUME_KEYS) + (None,)
    c = np.ascontiguousarray(scene.coords).astype(np.int64).reshape(-1, 3)
    order = np.lexsort((c[:, 2], c[:, 1], c[:, 0]))
    return (c[order],) + tuple(a[k][order] for k in VOLUME_KEYS) + (order,)


def write_scene(path, tsdf, semantic, instance, coords=None, **head):
    """THE writer: [X,Y,Z] volumes -> the dense layout; with coords [M,3], rows -> the sparse one.  **head: origin,
    voxel_size (dims with rows) and whatever else the file is to carry.  Written through a file object, so numpy appends no
    .npz to the name."""
    if coords is None:
        body = {"tsdf": tsdf, "semantic": semantic, "instance": instance}
    else:
        body = {"sparse_coords": coords, "sparse_tsdf": tsdf, "sparse_semantic": semantic, "sparse_instance": instance}
    with open(path, "wb") as fh:
        np.savez_compressed(fh, **head, **body)


def read_scene_list(path):
    """a text file, one scene name per line (blank lines skipped)"""
    with open(path, "r", encoding="utf-8") as fh:
        return [line.strip() for line in fh if line.strip()]


# ---------------------------------------------------------------------------------------------------------------- PLY

_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
              "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
              "double": "f8", "float64": "f8"}


def read_ply(path):
    """PLY (binary little / big endian or ASCII) -> (vertices f32[N,3], faces int32[M,3]); polygons are fanned into
    triangles, elements other than vertex / face are skipped.  numpy only."""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.find(b"end_header")
    if not data.startswith(b"ply") or end < 0:
        raise ValueError(f"{path}: not a PLY file")
    body = end + len(b"end_header")
    body += 2 if data[body:body + 2] == b"\r\n" else 1
    fmt, elements = None, []
    for line in data[:end].decode("ascii", "replace").splitlines():
        tok = line.split()
        if not tok or tok[0] in ("ply", "comment", "obj_info"):
            continue
        if tok[0] == "format":
            fmt = tok[1]
        elif tok[0] == "element":
            elements.append((tok[1], int(tok[2]), []))
        elif tok[0] == "property":
            if tok[1] == "list":
                elements[-1][2].append((tok[4], _PLY_TYPES[tok[2]], _PLY_TYPES[tok[3]]))
            else:
                elements[-1][2].append((tok[2], _PLY_TYPES[tok[1]], None))
    if fmt not in ("ascii", "binary_little_endian", "binary_big_endian"):
        raise ValueError(f"{path}: unsupported PLY format {fmt}")
    verts, faces = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    if fmt == "ascii":
        lines = data[body:].decode("ascii").split("\n")
        li = 0
        for name, count, props in elements:
            rows = []
            for _ in range(count):
                while not lines[li].strip():
                    li += 1
                rows.append(lines[li].split())
                li += 1
            if name == "vertex":
                names = [p[0] for p in props]
                arr = np.array([[float(r[names.index(a)]) for a in "xyz"] for r in rows], np.float64).reshape(-1, 3)
                verts = arr.astype(np.float32)
            elif name == "face":
                faces = _fan(_ascii_lists(rows, props))
        return verts, faces
    order = "<" if fmt == "binary_little_endian" else ">"
    off = body
    for name, count, props in elements:
        if all(p[2] is None for p in props):
            dt = np.dtype([(p[0], order + p[1]) for p in props])
            rec = np.frombuffer(data, dt, count, off)
            off += dt.itemsize * count
            if name == "vertex":
                verts = np.stack([rec[a] for a in "xyz"], 1).astype(np.float32)
            continue
        # an element with list properties: one structured read when every list holds three items (triangle meshes)
        fields = []
        for p in props:
            fields += [(p[0], order + p[1])] if p[2] is None else [(p[0] + "_n", order + p[1]), (p[0], order + p[2], (3,))]
        dt3 = np.dtype(fields)
        if off + dt3.itemsize * count <= len(data):
            rec = np.frombuffer(data, dt3, count, off)
            if all((rec[p[0] + "_n"] == 3).all() for p in props if p[2]):
                off += dt3.itemsize * count
                if name == "face":
                    key = [p[0] for p in props if p[2] and p[0] in ("vertex_indices", "vertex_index")]
                    faces = np.ascontiguousarray(rec[key[0]], np.int32).reshape(-1, 3) if key else faces
                continue
        polys = []
        for _ in range(count):
            for p in props:
                if p[2] is None:
                    off += np.dtype(p[1]).itemsize
                    continue
                n = int(np.frombuffer(data, order + p[1], 1, off)[0])
                off += np.dtype(p[1]).itemsize
                items = np.frombuffer(data, order + p[2], n, off)
                off += np.dtype(p[2]).itemsize * n
                if p[0] in ("vertex_indices", "vertex_index"):
                    polys.append(items.astype(np.int64))
        if name == "face":
            faces = _fan(polys)
    return verts, faces


def _ascii_lists(rows, props):
    polys = []
    for r in rows:
        k = 0
        for p in props:
            if p[2] is None:
                k += 1
                continue
            n = int(float(r[k]))
            items = [int(float(x)) for x in r[k + 1:k + 1 + n]]
            k += 1 + n
            if p[0] in ("vertex_indices", "vertex_index"):
                polys.append(np.array(items, np.int64))
    return polys


def _fan(polys):
    tris = [np.stack([np.full(len(p) - 2, p[0]), p[1:-1], p[2:]], 1) for p in polys if len(p) >= 3]
    return np.concatenate(tris).astype(np.int32) if tris else np.zeros((0, 3), np.int32)


def load_mesh(mesh_or_path):
    """path / {vertices, faces} dict / (verts, faces) -> (verts f32[N,3], faces int32[M,3]) as numpy or tensors"""
    if isinstance(mesh_or_path, (str, os.PathLike)):
        return read_ply(mesh_or_path)
    if isinstance(mesh_or_path, dict):
        return mesh_or_path["vertices"], mesh_or_path["faces"]
    return mesh_or_path


def export_ply(mesh, path):
    """binary little-endian PLY with normals and (when present) RGB vertex colours — what trimesh's mesh.export writes.
    A mesh with "edges" int[E,2] is a wireframe instead: vertices without normals, no faces, an `edge` element of
    vertex1 / vertex2 (the boxes of scene_objects)."""
    if mesh.get("edges") is not None:
        return _export_edges_ply(mesh, path)
    v = np.ascontiguousarray(mesh["vertices"], np.float32)
    n = np.ascontiguousarray(mesh["vertex_normals"], np.float32)
    f = np.ascontiguousarray(mesh["faces"], np.int32)
    col = mesh.get("vertex_colors")
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
    if col is not None:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    rec = np.zeros(len(v), dtype=fields)
    rec["x"], rec["y"], rec["z"] = v[:, 0], v[:, 1], v[:, 2]
    rec["nx"], rec["ny"], rec["nz"] = n[:, 0], n[:, 1], n[:, 2]
    if col is not None:
        rec["red"], rec["green"], rec["blue"] = col[:, 0], col[:, 1], col[:, 2]
    frec = np.zeros(len(f), dtype=[("n", "u1"), ("a", "<i4"), ("b", "<i4"), ("c", "<i4")])
    frec["n"], frec["a"], frec["b"], frec["c"] = 3, f[:, 0], f[:, 1], f[:, 2]
    names = {"<f4": "float", "u1": "uchar"}
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}"]
    head += [f"property {names[t]} {k}" for k, t in fields]
    head += [f"element face {len(f)}", "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as fh:
        fh.write(("\n".join(head) + "\n").encode("ascii"))
        fh.write(rec.tobytes())
        fh.write(frec.tobytes())


def _export_edges_ply(mesh, path):
    v = np.ascontiguousarray(mesh["vertices"], np.float32).reshape(-1, 3)
    e = np.ascontiguousarray(mesh["edges"], np.int32).reshape(-1, 2)
    col = mesh.get("vertex_colors")
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")] + ([("red", "u1"), ("green", "u1"), ("blue", "u1")] if col is not None else [])
    rec = np.zeros(len(v), dtype=fields)
    rec["x"], rec["y"], rec["z"] = v[:, 0], v[:, 1], v[:, 2]
    if col is not None:
        col = np.asarray(col).reshape(-1, 3)
        rec["red"], rec["green"], rec["blue"] = col[:, 0], col[:, 1], col[:, 2]
    erec = np.zeros(len(e), dtype=[("vertex1", "<i4"), ("vertex2", "<i4")])
    erec["vertex1"], erec["vertex2"] = e[:, 0], e[:, 1]
    names = {"<f4": "float", "u1": "uchar"}
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}"]
    head += [f"property {names[t]} {k}" for k, t in fields]
    head += [f"element edge {len(e)}", "property int vertex1", "property int vertex2", "end_header"]
    with open(path, "wb") as fh:
        fh.write(("\n".join(head) + "\n").encode("ascii"))
        fh.write(rec.tobytes())
        fh.write(erec.tobytes())


# ----------------------------------------------------------------------------------- a ScanNet-layout scene directory
# <root>/pose/pose_<i>.txt, intrinsic/intrinsic_{depth,color}.txt, depth/depth_<i>.png, color/color_<i>.jpg.  np.loadtxt is
# called without a delimiter: splitting at any whitespace reads every file that delimiter=" " reads, to the same values,
# and files written with tabs or a trailing space besides.

def intrinsic(root, sensor):
    """intrinsic/intrinsic_<sensor>.txt ("depth" or "color") -> K float64[3,3]"""
    return np.loadtxt(os.path.join(root, "intrinsic", f"intrinsic_{sensor}.txt"), dtype=np.float64)[:3, :3]


def pose(root, i):
    """pose/pose_<i>.txt -> camera -> world, float64[4,4] (an untracked frame's is not finite)"""
    return np.loadtxt(os.path.join(root, "pose", f"pose_{int(i):d}.txt"), dtype=np.float64).reshape(4, 4)


def count_depth_frames(root):
    """the frame count of the evaluation and the ground-truth tools: the depth images (tools/simple_loader.py)"""
    return len([f for f in os.listdir(os.path.join(root, "depth")) if f.endswith(".png")])


def pose_frame_ids(root, every=1):
    """the frames of the rendering and colouring tools: 0, every, 2 every, ... below the number of pose_*.txt files"""
    n = len([f for f in os.listdir(os.path.join(root, "pose")) if f.startswith("pose_") and f.endswith(".txt")])
    return list(range(0, n, max(int(every), 1)))


def depth_metres(path, max_depth):
    """a 16-bit PNG in millimetres -> f32[H,W] metres, values above max_depth zeroed (tools/simple_loader.py:44-47)"""
    from PIL import Image
    with Image.open(path) as im:
        depth = np.asarray(im).astype(np.float32)
    depth /= 1000.
    depth[depth > max_depth] = 0
    return depth
