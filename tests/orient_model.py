"""The numpy model of the EXIF orientation (include/hjd.h, hjd_orient_item):
orient(S, o) builds the displayed image D from the table, element by element
of the index arithmetic, and oriented_roi maps a rectangle on D to the one on
S that holds the same pixels."""
import numpy as np


def tiff_block(order, entries, ifd_offset=8, count=None, magic=42, next_ifd=True):
    """A TIFF header + IFD0: order b"II" / b"MM", entries (tag, type, count,
    value) with the value a SHORT or LONG in the value field's first bytes."""
    e = "<" if order == b"II" else ">"
    out = order + int(magic).to_bytes(2, "little" if e == "<" else "big") + \
        int(ifd_offset).to_bytes(4, "little" if e == "<" else "big")
    out += b"\0" * (ifd_offset - 8 if ifd_offset >= 8 else 0)
    out += np.array([len(entries) if count is None else count], e + "u2").tobytes()
    for tag, typ, cnt, value in entries:
        out += np.array([tag, typ], e + "u2").tobytes() + np.array([cnt], e + "u4").tobytes()
        out += (np.array([value, 0], e + "u2") if typ == 3 else np.array([value], e + "u4")).tobytes()
    return out + (b"\0\0\0\0" if next_ifd else b"")


def app1(payload):
    """An APP1 segment of this payload (its length field consistent with it)."""
    return b"\xff\xe1" + (len(payload) + 2).to_bytes(2, "big") + payload


def exif_app1(tiff):
    return app1(b"Exif\0\0" + tiff)


def with_segments(jpeg, *segments):
    """The file with these segments inserted right after its SOI."""
    assert jpeg[:2] == b"\xff\xd8"
    return jpeg[:2] + b"".join(segments) + jpeg[2:]


def pil_jpeg(w, h, sub, seed, orientation=None, gray=False, q=90):
    """A Pillow-written JPEG (a gradient plus noise), with Pillow's own EXIF
    block carrying the orientation if one is given."""
    import io

    from PIL import Image
    rng = np.random.default_rng(seed)
    x = np.linspace(0, 255, w)[None, :, None]
    y = np.linspace(0, 255, h)[:, None, None]
    img = np.clip(x * [1, 0, 0.5] + y * [0, 1, 0.5] + rng.normal(0, 20.0, (h, w, 3)), 0, 255).astype(np.uint8)
    im = Image.fromarray(img)
    if gray:
        im = im.convert("L")
    kw = {}
    if orientation is not None:
        exif = Image.Exif()
        exif[0x0112] = int(orientation)
        kw["exif"] = exif.tobytes()
    b = io.BytesIO()
    im.save(b, format="JPEG", quality=q, subsampling=sub, **kw)
    return b.getvalue()


def oriented_size(w, h, o):
    """(W, H) of D for a stored w x h."""
    return (h, w) if o >= 5 else (w, h)


def orient(S, o):
    """S: (..., h, w); returns D (..., H, W) of the table's row o, a new array."""
    assert 1 <= o <= 8
    h, w = S.shape[-2:]
    dw, dh = oriented_size(w, h, o)
    i, j = np.meshgrid(np.arange(dh), np.arange(dw), indexing="ij")   # D[i][j]
    rows, cols = {
        1: (i, j),
        2: (i, w - 1 - j),
        3: (h - 1 - i, w - 1 - j),
        4: (h - 1 - i, j),
        5: (j, i),
        6: (h - 1 - j, i),
        7: (h - 1 - j, w - 1 - i),
        8: (j, w - 1 - i),
    }[o]
    return np.ascontiguousarray(S[..., rows, cols])


def oriented_roi(width, height, o, roi):
    """The stored (x, y, w, h) of a display rectangle, derived from the table:
    the display rows / columns are mapped through the same index arithmetic
    and the extremes taken."""
    x, y, w, h = roi
    dw, dh = oriented_size(width, height, o)
    assert 0 <= x and 0 <= y and w >= 1 and h >= 1 and x + w <= dw and y + h <= dh
    idx = np.arange(width * height).reshape(height, width)
    part = orient(idx, o)[y:y + h, x:x + w]
    rows, cols = part // width, part % width
    return (int(cols.min()), int(rows.min()), int(cols.max() - cols.min() + 1), int(rows.max() - rows.min() + 1))
