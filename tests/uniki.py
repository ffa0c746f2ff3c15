"""Test-side reader of `.uniki` files and the expected output of the inspection commands, written from the reference's format and
rules alone (index/serialization.go:159-300 file layout; cmd/index-density.go:150-268; cmd/ref-info.go:107-149; util-hash.go:55): nothing here
calls the code under test, the counts are recounted from the file's bytes with numpy."""
import math
import struct

import numpy as np


def read_header(path):
    """dict(k, canonical, num_hashes, num_sigs, names, gsizes, indices, sizes, row_bytes, offset0) of a .uniki file"""
    with open(path, "rb") as f:
        data = f.read()
    assert data[:8] == b".kmcpidx", path
    version, k, flags, num_hashes = data[8], data[9], data[10], data[11]
    assert version == 4
    at = 12
    (num_sigs,) = struct.unpack_from(">Q", data, at)
    at += 8
    (n,) = struct.unpack_from(">I", data, at)
    at += 4
    names = []
    for _ in range(n):
        (ln,) = struct.unpack_from(">I", data, at)
        at += 4
        names.append(data[at:at + ln].split(b"\n")[0].decode())
        at += ln
    gsizes, indices = [], []
    (ng,) = struct.unpack_from(">I", data, at)
    at += 4
    for _ in range(ng):
        (m,) = struct.unpack_from(">I", data, at)
        at += 4
        vals = struct.unpack_from(">%dQ" % m, data, at)
        at += 8 * m
        gsizes.append(vals[0] if m else 0)
    (ni,) = struct.unpack_from(">I", data, at)
    at += 4
    for _ in range(ni):
        (m,) = struct.unpack_from(">I", data, at)
        at += 4
        vals = struct.unpack_from(">%dI" % m, data, at)
        at += 4 * m
        indices.append(vals[0] if m else 0)
    sizes = list(struct.unpack_from(">%dQ" % n, data, at))
    at += 8 * n
    row_bytes = (n + 7) // 8
    assert len(data) - at == num_sigs * row_bytes, (path, len(data) - at, num_sigs, row_bytes)
    return dict(k=k, canonical=bool(flags & 1), num_hashes=num_hashes, num_sigs=num_sigs, names=names, gsizes=gsizes, indices=indices, sizes=sizes,
                row_bytes=row_bytes, offset0=at)


def read_rows(path, h=None):
    """the bit matrix of a .uniki file as uint8 [num_sigs, row_bytes]"""
    h = h or read_header(path)
    return np.fromfile(path, dtype=np.uint8, offset=h["offset0"]).reshape(h["num_sigs"], h["row_bytes"])


def recount(rows, n_cols, bin_rows, first_row=0, n_rows=0):
    """set bits per (column, bin) of rows first_row .. (n_rows of them, 0 = to the end), MSB of a byte = first column: uint32 [n_cols, n_bins]"""
    last = rows.shape[0] if n_rows == 0 else first_row + n_rows
    part = rows[first_row:last]
    n = part.shape[0]
    n_bins = (n + bin_rows - 1) // bin_rows
    out = np.zeros((n_cols, n_bins), dtype=np.uint32)
    # bin by bin over at most ~64 MB of unpacked bits at a time
    step = max(1, (64 << 20) // max(1, rows.shape[1] * 8 * bin_rows))
    for b0 in range(0, n_bins, step):
        b1 = min(n_bins, b0 + step)
        bits = np.unpackbits(part[b0 * bin_rows:b1 * bin_rows], axis=1, bitorder="big")[:, :n_cols]
        for b in range(b0, b1):
            out[:, b] = bits[(b - b0) * bin_rows:(b - b0 + 1) * bin_rows].sum(axis=0, dtype=np.uint64)
    return out


def density_bins(num_sigs, bins=1024, bin_size=0):
    """(bins, binSize) as index-density.go:150-155 derives them"""
    if bin_size > 0:
        return num_sigs // bin_size + 1, bin_size
    return bins, num_sigs // bins


def density_tsv(path, bins=1024, bin_size=0):
    """the text `kmcp utils index-density` prints: floor(NumSigs / binSize) counts per column, the trailing bin never printed (:225-241)"""
    h = read_header(path)
    bins, bin_size = density_bins(h["num_sigs"], bins, bin_size)
    n_full = h["num_sigs"] // bin_size
    counts = recount(read_rows(path, h), len(h["names"]), bin_size, 0, n_full * bin_size)
    lines = ["target\tchunkIdx\tbins\tbinSize\tcounts\n"]
    for i, name in enumerate(h["names"]):
        lines.append("%s\t%d\t%d\t%d\t%s\n" % (name, h["indices"][i] & 65535, bins, bin_size, ",".join(str(int(c)) for c in counts[i])))
    return "".join(lines)


def density_pgm(path, bins=1024, bin_size=0):
    """the image of index-density.go:263-268 as a binary PGM: width bins, height #names, pixel 255 - uint8(float64(c) * (255 / binSize)) for
    every entry of a column's counts — the full bins and the trailing one (empty when binSize divides NumSigs) — that lies inside the
    image, 0 elsewhere"""
    h = read_header(path)
    bins, bin_size = density_bins(h["num_sigs"], bins, bin_size)
    n_names = len(h["names"])
    full = recount(read_rows(path, h), n_names, bin_size)
    n_full = h["num_sigs"] // bin_size
    entries = np.zeros((n_names, n_full + 1), dtype=np.float64)
    entries[:, :full.shape[1]] = full
    r = 255.0 / float(bin_size)
    px = (255 - np.floor(entries * r).astype(np.int64)).astype(np.uint8)
    img = np.zeros((n_names, bins), dtype=np.uint8)
    w = min(bins, n_full + 1)
    img[:, :w] = px[:, :w]
    return b"P5\n%d %d\n255\n" % (bins, n_names) + img.tobytes()


def calc_fpr(n, num_hashes, num_sigs):
    """CalcFPR (util-hash.go:55)"""
    return math.pow(1 - math.pow(math.e, float(-num_hashes) * float(n) / float(num_sigs)), float(num_hashes))


def ref_info_rows(db_dir, files):
    """[(file, i, target, chunkIdx, chunks, kmers, fpr, num_sigs, num_hashes)] for the .uniki files of one R* directory, in `files` order"""
    import os
    out = []
    for fn in files:
        h = read_header(os.path.join(db_dir, fn))
        for i, n in enumerate(h["sizes"]):
            idx = h["indices"][i]
            out.append((fn, i + 1, h["names"][i], idx & 65535, idx >> 16, n, calc_fpr(n, h["num_hashes"], h["num_sigs"]), h["num_sigs"], h["num_hashes"]))
    return out


def db_files(db_dir):
    """the `files` list of <db_dir>/__db.yml"""
    import os
    files, on = [], False
    for line in open(os.path.join(db_dir, "__db.yml")):
        s = line.strip()
        if s.startswith("files:"):
            on = True
            continue
        if on:
            if s.startswith("- "):
                files.append(s[2:].strip().strip('"').strip("'"))
            elif s and not s.startswith("#"):
                on = False
    return files
