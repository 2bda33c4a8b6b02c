"""Writes refvsr_amd/csrc/colormap_table.h: matplotlib's 256-entry `inferno` table as the bytes the reference's confidence-map
images hold (evaluation/eval_quan_conf_map.py:20,83-84,126,150).  Run once where matplotlib is installed; the library and the
package never import matplotlib.

Entry i is what the reference's chain makes of colour-table index i:
    colormap(x)[:, :, :3]   float64 rows of the 256-entry table
    torch.Tensor(...)       -> float32
    x * 255                 float32 product
    cv2.imwrite             saturate_cast<uchar>: round to nearest (ties to even), saturate
i.e. u8[i][c] = rint(float32(float32(lut64[i][c]) * 255)).

    python tools/gen_colormap_table.py            # rewrites the header
    python tools/gen_colormap_table.py --check    # compares the header's bytes with matplotlib's
"""
import hashlib
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(HERE, '..', 'refvsr_amd', 'csrc', 'colormap_table.h')


def table_bytes():
    """uint8 [256, 3] from matplotlib's inferno, and the smallest distance of a float32 product from a rounding tie."""
    import matplotlib
    import matplotlib.pyplot as plt
    cmap = plt.get_cmap('inferno')
    lut64 = np.asarray(cmap(np.arange(256, dtype=np.int64)), dtype=np.float64)[:, :3]
    prod = lut64.astype(np.float32) * np.float32(255)
    assert prod.dtype == np.float32
    tie = float(np.abs(prod.astype(np.float64) - np.floor(prod.astype(np.float64)) - 0.5).min())
    return np.clip(np.rint(prod), 0, 255).astype(np.uint8), tie, matplotlib.__version__


def header_text(u8, version):
    digest = hashlib.sha256(u8.tobytes()).hexdigest()
    rows = []
    for i in range(0, 256, 4):
        rows.append('    ' + ' '.join('{%3d, %3d, %3d},' % tuple(int(v) for v in u8[j]) for j in range(i, i + 4)))
    return (
        "// The colour table of the confidence-map images: matplotlib's 256-entry `inferno` map as the bytes the reference writes,\n"
        "// u8[i][c] = rint(float32(float32(lut64[i][c]) * 255)) (evaluation/eval_quan_conf_map.py:20,83-84,126,150: colormap(x)[:, :, :3],\n"
        "// torch.Tensor -> float32, * 255 in float32, cv2.imwrite's round-to-nearest saturating cast).  Data from matplotlib (%s), written\n"
        "// by tools/gen_colormap_table.py -- do not edit.  sha256 of the 768 bytes in row-major RGB order:\n"
        "// %s\n"
        "// One definition for every kernel that colours a map: colormap.hip includes it once and owns its copy in constant memory.\n"
        "#pragma once\n\n"
        "struct ColormapTable { unsigned char v[256][3]; };\n"
        "static constexpr ColormapTable colormap_table() {\n"
        "    return ColormapTable{{\n%s\n    }};\n"
        "}\n" % (version, digest, '\n'.join(rows)))


def header_bytes(path=HEADER):
    """The 768 bytes a written header holds."""
    src = open(path).read()
    body = src[src.index('return ColormapTable{{'):]
    vals = [int(v) for t in re.findall(r'\{\s*(\d+),\s*(\d+),\s*(\d+)\}', body) for v in t]
    return np.array(vals, dtype=np.uint8).reshape(256, 3)


def main(argv):
    u8, tie, version = table_bytes()
    print('matplotlib %s: sha256 %s, nearest tie %.3g' % (version, hashlib.sha256(u8.tobytes()).hexdigest(), tie))
    if '--check' in argv:
        ok = np.array_equal(header_bytes(), u8)
        print('header %s' % ('matches' if ok else 'DIFFERS'))
        return 0 if ok else 1
    with open(HEADER, 'w') as fh:
        fh.write(header_text(u8, version))
    print('wrote %s' % os.path.normpath(HEADER))
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
