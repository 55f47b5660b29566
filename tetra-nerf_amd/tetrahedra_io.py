"""The `.th` tetrahedra file either side of the hot path.

Format (tetranerf/scripts/triangulate.py:68-75): a `torch.save`d dict
    {"cells": i32 [T,4], "vertices": f32 [V,3], "colors": u8 [V,4] (optional)}
read back by the model (tetranerf/nerfstudio/model.py:349-392): vertices go through the dataparser
transform ([x,1] @ T^T, then * scale), cells to int32, and -- with `initialize_colors` -- the field rows
1..3 are seeded from RGB (c*2/255 - 1) and row 0 from alpha."""
from __future__ import annotations

from pathlib import Path
from typing import Dict, Optional

import torch


def save_tetrahedra(path, vertices: torch.Tensor, cells: torch.Tensor, colors: Optional[torch.Tensor] = None) -> None:
    out = {"cells": cells.detach().cpu().int(), "vertices": vertices.detach().cpu().float()}
    if colors is not None:
        if colors.dtype != torch.uint8 or tuple(colors.shape) != (len(vertices), 4):
            raise ValueError("colors must be uint8 [num_vertices, 4]")
        out["colors"] = colors.detach().cpu()
    Path(path).absolute().parent.mkdir(parents=True, exist_ok=True)
    torch.save(out, str(path))


def load_tetrahedra(path, dataparser_transform: Optional[torch.Tensor] = None,
                    dataparser_scale: Optional[float] = None) -> Dict[str, torch.Tensor]:
    """-> {"vertices": f32 [V,3] (transformed like model.py:355-373), "cells": i32 [T,4], "colors": u8 [V,4]?}."""
    path = Path(path)
    if not path.exists():
        raise RuntimeError(f"Specified tetrahedra path {path} does not exist")
    t = torch.load(str(path), map_location=torch.device("cpu"))
    vertices = t["vertices"].float()
    if dataparser_transform is not None:
        hom = torch.cat((vertices, torch.ones_like(vertices[..., :1])), -1)
        vertices = hom @ dataparser_transform.T.to(vertices.dtype)
    if dataparser_scale is not None:
        vertices = vertices * dataparser_scale
    out = {"vertices": vertices.contiguous(), "cells": t["cells"].int().contiguous()}
    if "colors" in t:
        out["colors"] = t["colors"]
    return out


def init_field_from_colors(field: torch.Tensor, colors: torch.Tensor) -> None:
    """model.py:380-386: field [64,V]; rows 1..3 <- RGB in [-1,1], row 0 <- alpha in [-1,1]."""
    if colors.dtype != torch.uint8 or tuple(colors.shape) != (field.shape[1], 4):
        raise ValueError("colors must be uint8 [num_vertices, 4]")
    c = colors.float().to(field.device) * 2.0 / 255.0 - 1.0
    field.data[1:4, :] = c[:, :3].T
    field.data[0, :] = c[:, 3]


# ---- triangle meshes (render.extract_mesh): binary little-endian PLY, the format every mesh viewer reads

def save_mesh_ply(path, positions, triangles, colors=None) -> None:
    """positions f32 [N, 3], triangles integer [M, 3] (rows of positions), colors uint8 [N, 3] or None (tensors or arrays) ->
    a binary_little_endian PLY: vertices x y z [red green blue], faces as `list uchar int vertex_indices`."""
    import numpy as np

    def host(x):
        return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)

    p, t = np.ascontiguousarray(host(positions), "<f4"), np.ascontiguousarray(host(triangles)).astype("<i4")
    if p.ndim != 2 or p.shape[1] != 3 or t.ndim != 2 or t.shape[1] != 3:
        raise ValueError("positions must be [num_vertices, 3] and triangles [num_triangles, 3]")
    if len(t) and (t.min() < 0 or t.max() >= len(p)):
        raise ValueError("triangles names a vertex that is not in positions")
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if colors is not None:
        c = host(colors)
        if c.dtype != np.uint8 or c.shape != (len(p), 3):
            raise ValueError("colors must be uint8 [num_vertices, 3]")
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    vertex = np.zeros(len(p), np.dtype(fields))
    vertex["x"], vertex["y"], vertex["z"] = p[:, 0], p[:, 1], p[:, 2]
    if colors is not None:
        vertex["red"], vertex["green"], vertex["blue"] = c[:, 0], c[:, 1], c[:, 2]
    face = np.zeros(len(t), np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
    face["n"], face["v"] = 3, t
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {len(p)}", "property float x", "property float y",
              "property float z"]
    if colors is not None:
        header += ["property uchar red", "property uchar green", "property uchar blue"]
    header += [f"element face {len(t)}", "property list uchar int vertex_indices", "end_header"]
    Path(path).absolute().parent.mkdir(parents=True, exist_ok=True)
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\n").encode("ascii"))
        f.write(vertex.tobytes())
        f.write(face.tobytes())


def load_mesh_ply(path) -> Dict[str, torch.Tensor]:
    """-> {"positions": f32 [N, 3], "triangles": i32 [M, 3], "colors": u8 [N, 3] or None} of a PLY written by save_mesh_ply (binary
    little-endian, float x y z then optional uchar red green blue, triangular faces as `list uchar int`); anything else raises."""
    import numpy as np

    raw = Path(path).read_bytes()
    end = raw.find(b"end_header\n")
    if not raw.startswith(b"ply\n") or end < 0:
        raise ValueError(f"{path}: not a PLY file")
    lines = raw[:end].decode("ascii").split("\n")[1:]
    if not lines or lines[0] != "format binary_little_endian 1.0":
        raise ValueError(f"{path}: only binary_little_endian 1.0 is read")
    counts, props, element = {}, {}, None
    for line in lines[1:]:
        words = line.split()
        if not words or words[0] in ("comment", "obj_info"):
            continue
        if words[0] == "element":
            element = words[1]
            counts[element], props[element] = int(words[2]), []
        elif words[0] == "property" and element is not None:
            props[element].append(tuple(words[1:]))
    xyz, rgb = [("float", a) for a in "xyz"], [("uchar", a) for a in ("red", "green", "blue")]
    if list(counts) != ["vertex", "face"] or props["vertex"] not in (xyz, xyz + rgb) or \
            props["face"] != [("list", "uchar", "int", "vertex_indices")]:
        raise ValueError(f"{path}: not the layout save_mesh_ply writes")
    colored = props["vertex"] == xyz + rgb
    vdt = np.dtype([("p", "<f4", (3,))] + ([("c", "u1", (3,))] if colored else []))
    fdt = np.dtype([("n", "u1"), ("v", "<i4", (3,))])
    body = raw[end + len(b"end_header\n"):]
    nv, nf = counts["vertex"], counts["face"]
    if len(body) != nv * vdt.itemsize + nf * fdt.itemsize:
        raise ValueError(f"{path}: the body is {len(body)} bytes, the header promises {nv * vdt.itemsize + nf * fdt.itemsize}")
    vertex = np.frombuffer(body, vdt, nv)
    face = np.frombuffer(body, fdt, nf, offset=nv * vdt.itemsize)
    if nf and not (face["n"] == 3).all():
        raise ValueError(f"{path}: a face that is not a triangle")
    return {"positions": torch.from_numpy(np.array(vertex["p"])), "triangles": torch.from_numpy(np.array(face["v"])),
            "colors": torch.from_numpy(np.array(vertex["c"])) if colored else None}
