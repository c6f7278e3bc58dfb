"""Triangle meshes from .off and .ply files: the input of ds_mesh_to_pc (the reference reads them with pyntcloud).

read_mesh(path) -> (float64 (V,3) vertices, int32 (F,3) triangles).  Polygons are fan-triangulated: (i0, ij, ij+1) for
j = 1 .. k-2.  The triangles follow the file: face by face, and the fan of a face in order of j (the sampled bits depend on this
order).  A face with fewer than 3 vertices, an index outside [0, V) or a malformed file raises ValueError naming the file.
  - .off: the header line `OFF`, ModelNet's glued `OFF490 518 0`, `#` comments, blank lines, extra values after a vertex's three
    coordinates or after a face's indices (colours);
  - .ply: ascii, binary_little_endian and binary_big_endian; the `vertex` element's x, y, z of any numeric type, a `face` element
    whose list property is named vertex_indices or vertex_index (any count / index type); other elements and properties are skipped.
pc_io.read_ply (vertex-only clouds) is separate and unchanged.
"""
import os

import numpy as np

from .pc_io import _PLY_TYPES

_FACE_LISTS = ('vertex_indices', 'vertex_index')


def read_mesh(path):
    ext = os.path.splitext(path)[1].lower()
    with open(path, 'rb') as f:
        head = f.read(4)
    if ext == '.off' or (ext != '.ply' and head[:3] in (b'OFF', b'off')):
        v, polys = _read_off(path)
    elif ext == '.ply' or head[:3] == b'ply':
        v, polys = _read_ply_mesh(path)
    else:
        raise ValueError(f'{path}: unknown mesh format (expected .off or .ply)')
    return v, _triangulate(path, polys, v.shape[0])


def _triangulate(path, polys, nv):
    """polys: groups (k, (m, k) index array, (m,) face numbers in the file) -> (F,3) int32 fans in file order (face by face, then
    j = 1 .. k-2 within a face), checked."""
    tris, keys = [], []
    kmax = max([k for k, _, _ in polys] + [3])
    for k, idx, faces in polys:
        if k < 3:
            raise ValueError(f'{path}: a face has {k} vertices (at least 3 are needed)')
        if len(idx) and (idx.min() < 0 or idx.max() >= nv):
            raise ValueError(f'{path}: face index outside [0, {nv})')
        idx = idx.astype(np.int64)
        for j in range(1, k - 1):
            tris.append(np.stack([idx[:, 0], idx[:, j], idx[:, j + 1]], 1))
            keys.append(np.asarray(faces, np.int64) * kmax + j)
    if not tris:
        return np.zeros((0, 3), np.int32)
    order = np.argsort(np.concatenate(keys), kind='stable')
    return np.ascontiguousarray(np.concatenate(tris)[order], np.int32)


def _group_faces(rows):
    """Index lists of varying length -> [(k, (m, k) array, (m,) face numbers)]: the faces of each vertex count, in file order."""
    by_k = {}
    for i, r in enumerate(rows):
        by_k.setdefault(len(r), ([], []))
        by_k[len(r)][0].append(r)
        by_k[len(r)][1].append(i)
    return [(k, np.asarray(g, np.int64).reshape(len(g), k), np.asarray(f, np.int64)) for k, (g, f) in by_k.items()]


def _read_off(path):
    with open(path, 'r', encoding='ascii', errors='replace') as f:
        lines = [ln.split('#', 1)[0].split() for ln in f]
    lines = [t for t in lines if t]
    if not lines or not lines[0][0].upper().startswith('OFF'):
        raise ValueError(f'{path}: not an OFF file')
    first = lines[0]
    rest = [first[0][3:]] + first[1:] if len(first[0]) > 3 else first[1:]      # ModelNet: `OFF490 518 0`
    rest = [t for t in rest if t]
    pos = 1
    if not rest:
        if len(lines) < 2:
            raise ValueError(f'{path}: missing the vertex / face counts')
        rest, pos = lines[1], 2
    try:
        nv, nf = int(rest[0]), int(rest[1])
    except (ValueError, IndexError):
        raise ValueError(f'{path}: bad OFF counts {rest!r}') from None
    if len(lines) < pos + nv + nf:
        raise ValueError(f'{path}: {nv} vertices and {nf} faces announced, the file ends early')
    try:
        v = np.array([t[:3] for t in lines[pos:pos + nv]], np.float64).reshape(nv, 3)
        rows = []
        for t in lines[pos + nv:pos + nv + nf]:
            k = int(t[0])
            if len(t) < 1 + k:
                raise ValueError
            rows.append([int(x) for x in t[1:1 + k]])
    except ValueError:
        raise ValueError(f'{path}: malformed vertex or face line') from None
    return v, _group_faces(rows)


def _ply_header(path, f):
    if f.readline().strip() != b'ply':
        raise ValueError(f'{path}: not a PLY file')
    fmt, elements = None, []
    while True:
        line = f.readline()
        if not line:
            raise ValueError(f'{path}: unexpected end of header')
        tok = line.decode('ascii', 'replace').split()
        if not tok or tok[0] in ('comment', 'obj_info'):
            continue
        if tok[0] == 'format':
            fmt = tok[1]
        elif tok[0] == 'element':
            elements.append((tok[1], int(tok[2]), []))
        elif tok[0] == 'property':
            if not elements:
                raise ValueError(f'{path}: property outside an element')
            try:
                prop = (tok[4], 'list', _PLY_TYPES[tok[2]], _PLY_TYPES[tok[3]]) if tok[1] == 'list' else (tok[2], _PLY_TYPES[tok[1]])
            except (KeyError, IndexError):
                raise ValueError(f'{path}: unsupported property line {line!r}') from None
            elements[-1][2].append(prop)
        elif tok[0] == 'end_header':
            break
    if fmt not in ('ascii', 'binary_little_endian', 'binary_big_endian'):
        raise ValueError(f'{path}: unsupported PLY format {fmt!r}')
    return fmt, elements


def _read_ply_mesh(path):
    with open(path, 'rb') as f:
        fmt, elements = _ply_header(path, f)
        body = f.read()
    names = [e[0] for e in elements]
    if 'vertex' not in names or 'face' not in names:
        raise ValueError(f'{path}: a mesh needs a vertex and a face element')
    face_props = elements[names.index('face')][2]
    if not any(p[0] in _FACE_LISTS and p[1] == 'list' for p in face_props):
        raise ValueError(f'{path}: the face element has no vertex_indices / vertex_index list')
    vprops = [p[0] for p in elements[names.index('vertex')][2]]
    if not all(c in vprops for c in 'xyz'):
        raise ValueError(f'{path}: the vertex element lacks x, y or z')
    data = _parse_ascii(path, body, elements) if fmt == 'ascii' else \
        _parse_binary(path, body, elements, '<' if fmt == 'binary_little_endian' else '>')
    vert = data['vertex']
    v = np.stack([np.asarray(vert[c], np.float64) for c in 'xyz'], 1).reshape(-1, 3)
    return v, data['face']


def _parse_ascii(path, body, elements):
    lines = [ln.split() for ln in body.decode('ascii', 'replace').splitlines()]
    lines = [t for t in lines if t]
    out, pos = {}, 0
    for name, count, props in elements:
        rows = lines[pos:pos + count]
        if len(rows) < count:
            raise ValueError(f'{path}: element {name} announces {count} rows, the file ends early')
        pos += count
        if name == 'vertex':
            cols = {}
            for j, p in enumerate(props):
                if p[1] == 'list':
                    raise ValueError(f'{path}: list properties on vertices are not supported')
                cols[p[0]] = np.array([float(r[j]) for r in rows], np.float64) if count else np.zeros(0)
            out['vertex'] = cols
        elif name == 'face':
            faces = []
            for r in rows:
                t, got = 0, None
                for p in props:
                    if p[1] == 'list':
                        k = int(r[t])
                        if p[0] in _FACE_LISTS and got is None:
                            got = [int(x) for x in r[t + 1:t + 1 + k]]
                        t += 1 + k
                    else:
                        t += 1
                faces.append(got)
            out['face'] = _group_faces(faces)
    return out


def _fixed_dtype(props, endian, counts):
    """Structured dtype of one row; counts[i] = the element count assumed for the i-th list property."""
    fields, li = [], 0
    for p in props:
        if p[1] == 'list':
            fields.append((f'{p[0]}__n', endian + p[2]))
            fields.append((p[0], endian + p[3], (counts[li],)))
            li += 1
        else:
            fields.append((p[0], endian + p[1]))
    return np.dtype(fields)


def _parse_binary(path, body, elements, endian):
    out, off = {}, 0
    for name, count, props in elements:
        lists = [p for p in props if p[1] == 'list']
        rec = None
        if not lists:
            dt = _fixed_dtype(props, endian, [])
            if off + dt.itemsize * count > len(body):
                raise ValueError(f'{path}: element {name} runs past the end of the file')
            rec = np.frombuffer(body, dt, count, off)
            off += dt.itemsize * count
        elif count:
            # fast path: every row has the counts of the first row (triangle meshes); else a row-by-row walk
            counts, o = [], off
            for p in props:
                if p[1] == 'list':
                    if o + np.dtype(p[2]).itemsize > len(body):
                        raise ValueError(f'{path}: element {name} runs past the end of the file')
                    k = int(np.frombuffer(body, endian + p[2], 1, o)[0])
                    counts.append(k)
                    o += np.dtype(p[2]).itemsize + k * np.dtype(p[3]).itemsize
                else:
                    o += np.dtype(p[1]).itemsize
            dt = _fixed_dtype(props, endian, counts)
            if off + dt.itemsize * count <= len(body):
                r = np.frombuffer(body, dt, count, off)
                if all((r[f'{p[0]}__n'] == k).all() for p, k in zip(lists, counts)):
                    rec = r
                    off += dt.itemsize * count
            if rec is None:
                rec, off = _walk_rows(path, body, off, name, count, props, endian)
        if name == 'vertex':
            out['vertex'] = {p[0]: rec[p[0]] for p in props} if count else {p[0]: np.zeros(0) for p in props}
        elif name == 'face':
            key = next(p[0] for p in props if p[1] == 'list' and p[0] in _FACE_LISTS)
            if not count:
                out['face'] = []
            elif isinstance(rec, np.ndarray):
                idx = np.asarray(rec[key]).reshape(count, -1)
                out['face'] = [(idx.shape[1], idx, np.arange(count))]
            else:
                out['face'] = _group_faces(rec[key])
    return out


def _walk_rows(path, body, off, name, count, props, endian):
    cols = {p[0]: [] for p in props}
    try:
        for _ in range(count):
            for p in props:
                if p[1] == 'list':
                    ct = np.dtype(endian + p[2])
                    k = int(np.frombuffer(body, ct, 1, off)[0])
                    off += ct.itemsize
                    it = np.dtype(endian + p[3])
                    cols[p[0]].append(np.frombuffer(body, it, k, off).tolist())
                    off += k * it.itemsize
                else:
                    dt = np.dtype(endian + p[1])
                    cols[p[0]].append(np.frombuffer(body, dt, 1, off)[0])
                    off += dt.itemsize
    except ValueError:
        raise ValueError(f'{path}: element {name} runs past the end of the file') from None
    return cols, off
