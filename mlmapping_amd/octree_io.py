"""The word stream of MLMap.export_octree as an OctoMap binary tree (.bt), and back.  Pure Python / numpy.

Compatibility with real OctoMap readers is UNPINNED: no OctoMap library was available where this was written, so the text header
and the bit layout below are written from memory of that format and have never been read by octomap's own `readBinary`.  What is
pinned (tests/test_octree_plan.py) is that `from_bt(to_bt(...))` gives the stream back and that `leaves_of` decodes a stream into
exactly the cubes mlm_export_octree reports.

The layout as remembered: a text header —

    # Octomap OcTree binary file
    # (comment lines)
    id OcTree
    size <number of nodes, inner nodes and leaves>
    res <edge of a voxel in metres>
    data

— then, per inner node in depth-first pre-order (children in order 0..7, child i taking bit 0 from x, bit 1 from y, bit 2 from z),
two bytes: children 0..3 in the first, 4..7 in the second, two bits per child from the low end: 00 unknown, 01 free leaf, 10 occupied
leaf, 11 a child with children.  That is mlm_export_octree's uint16 word, little-endian.  The tree has 16 levels below the root:
export with depth=16, whose key 2^15 is OctoMap's centre key.  A tree whose root is a leaf or absent has no word: OctoMap cannot
express a root without children other than as an empty tree.
"""
from __future__ import annotations

from typing import Dict, List, Tuple

import numpy as np

MAGIC = "# Octomap OcTree binary file"
NONE, FREE, OCC, INNER = 0, 1, 2, 3


def to_bt(words, n_leaves: int, res: float) -> bytes:
    """The .bt bytes of a word stream: header (size = inner nodes + leaves), then the words little-endian."""
    w = np.ascontiguousarray(np.asarray(words).reshape(-1), dtype="<u2")
    head = f"{MAGIC}\n# (feel free to add / change comments, but leave the first line as it is!)\n#\nid OcTree\nsize {len(w) + int(n_leaves)}\nres {float(res)!r}\ndata\n"
    return head.encode("ascii") + w.tobytes()


def from_bt(data: bytes) -> Dict[str, object]:
    """{"words": uint16 array, "size": int, "res": float, "id": str} of .bt bytes; raises ValueError on anything else."""
    if not data.startswith(MAGIC.encode("ascii")):
        raise ValueError("not an OctoMap binary tree: the first line differs")
    at, fields = 0, {}
    while True:
        end = data.find(b"\n", at)
        if end < 0:
            raise ValueError("no 'data' line in the header")
        line = data[at:end].decode("ascii").strip()
        at = end + 1
        if line == "data":
            break
        if not line or line.startswith("#"):
            continue
        key, _, value = line.partition(" ")
        fields[key] = value.strip()
    for key in ("id", "size", "res"):
        if key not in fields:
            raise ValueError(f"no '{key}' line in the header")
    if fields["id"] != "OcTree":
        raise ValueError(f"id {fields['id']!r} is not OcTree")
    body = data[at:]
    if len(body) % 2:
        raise ValueError("an odd number of payload bytes")
    return {"words": np.frombuffer(body, dtype="<u2").astype(np.uint16), "size": int(fields["size"]), "res": float(fields["res"]), "id": fields["id"]}


def leaves_of(words, depth: int) -> Tuple[np.ndarray, np.ndarray]:
    """Decode a word stream of a tree of `depth` levels: (leaf4 int32 (M, 4): lower corner x y z as voxel index and level, in stream
    order; leaf_class int8 (M,): 0 OCCUPIED, 1 FREE).  Raises ValueError if the stream ends early, has words left over or puts
    children below level 0."""
    w = np.asarray(words).reshape(-1)
    half = 1 << (depth - 1)
    rows: List[Tuple[int, int, int, int]] = []
    cls: List[int] = []
    if len(w) == 0:
        return np.zeros((0, 4), dtype=np.int32), np.zeros(0, dtype=np.int8)
    at = 0
    stack = [(0, 0, 0, depth, INNER)]  # key of the lower corner, level, label; the next node in pre-order on top
    while stack:
        kx, ky, kz, level, label = stack.pop()
        if label != INNER:
            rows.append((kx - half, ky - half, kz - half, level))
            cls.append(0 if label == OCC else 1)
            continue
        if at >= len(w):
            raise ValueError("the stream ends inside the tree")
        if level == 0:
            raise ValueError("an inner node at level 0")
        word = int(w[at])
        at += 1
        for i in reversed(range(8)):
            child = (word >> (2 * i)) & 3
            if child != NONE:
                stack.append((kx + ((i & 1) << (level - 1)), ky + (((i >> 1) & 1) << (level - 1)), kz + ((i >> 2) << (level - 1)), level - 1, child))
    if at != len(w):
        raise ValueError("words left over after the tree")
    return np.array(rows, dtype=np.int32).reshape(-1, 4), np.array(cls, dtype=np.int8)
