"""The 3-D reconstruction of a rollout as a file a viewer opens: a legacy-VTK STRUCTURED_POINTS data set with one float32
scalar per point, binary, big-endian -- what the reference writes with tvtk.ImageData + write_data
(visualization3D/pv_3Dview.py:184-192) and ParaView reads.  Host code, numpy only.

A volume [nz, ny, nx] in C order has x running fastest, which is the order the format wants and the reference's
np.stack(alpha_field_list, axis=2).ravel(order='F'): GrainRollout.grain_volume / orientation_volume go to the file as
they are."""
import numpy as np

_MAGIC = "# vtk DataFile Version 3.0"


def write_vtk(path, volume, spacing, name="theta_z"):
    """Write `volume` [nz, ny, nx] (anything np.asarray takes, or a torch tensor on any device) as float32 scalars `name` of a
    STRUCTURED_POINTS grid with DIMENSIONS nx ny nz.  spacing = (dx, dx, dz): the reference's in-plane mesh size
    dx = lxd / (fnx - 3) (pv_3Dview.py:156) and the distance of two layers dz = (height - base_width) / (frames - 1) * span
    (pv_3Dview.py:164) -- divided by 1 + interp_frames when the volume holds in-between layers; the origin is (0, 0, 0) as
    the reference's.  Returns the byte count."""
    if hasattr(volume, "detach"):
        volume = volume.detach().cpu().numpy()
    v = np.asarray(volume)
    if v.ndim != 3 or v.size == 0:
        raise ValueError(f"volume must be [nz, ny, nx] with points, got shape {v.shape}")
    spacing = [float(s) for s in spacing]
    if len(spacing) != 3 or not all(s > 0 and np.isfinite(s) for s in spacing):
        raise ValueError("spacing must be three positive numbers (dx, dy, dz)")
    name = str(name)
    if not name or any(ch.isspace() for ch in name):
        raise ValueError("the scalar's name must be one word")
    nz, ny, nx = v.shape
    header = "\n".join([
        _MAGIC, "grain structure", "BINARY", "DATASET STRUCTURED_POINTS", f"DIMENSIONS {nx} {ny} {nz}",
        "SPACING " + " ".join(repr(s) for s in spacing), "ORIGIN 0.0 0.0 0.0",
        f"POINT_DATA {v.size}", f"SCALARS {name} float", "LOOKUP_TABLE default", ""]).encode("ascii")
    body = np.ascontiguousarray(v, dtype=">f4").tobytes()
    with open(path, "wb") as f:
        f.write(header)
        f.write(body)
        f.write(b"\n")
    return len(header) + len(body) + 1


def read_vtk(path):
    """Read a file write_vtk wrote: {'volume': float32 [nz, ny, nx], 'spacing': (dx, dy, dz), 'origin': (..), 'name': str}."""
    with open(path, "rb") as f:
        raw = f.read()
    lines, at = [], 0
    while len(lines) < 10:
        end = raw.index(b"\n", at)
        lines.append(raw[at:end].decode("ascii"))
        at = end + 1
    if lines[0] != _MAGIC or lines[2] != "BINARY" or lines[3] != "DATASET STRUCTURED_POINTS":
        raise ValueError("not a binary legacy-VTK STRUCTURED_POINTS file")
    field = {ln.split()[0]: ln.split()[1:] for ln in lines[4:10]}
    nx, ny, nz = (int(s) for s in field["DIMENSIONS"])
    n = int(field["POINT_DATA"][0])
    if n != nx * ny * nz or field["SCALARS"][1] != "float" or field["LOOKUP_TABLE"] != ["default"]:
        raise ValueError("the header does not describe one float scalar per point")
    if len(raw) < at + 4 * n:
        raise ValueError("the file ends before its data does")
    volume = np.frombuffer(raw, dtype=">f4", count=n, offset=at).astype(np.float32).reshape(nz, ny, nx)
    return {"volume": volume, "spacing": tuple(float(s) for s in field["SPACING"]),
            "origin": tuple(float(s) for s in field["ORIGIN"]), "name": field["SCALARS"][0]}
