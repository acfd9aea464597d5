"""Write invertavatar_amd/csrc/mc_tables.h, the marching-cubes case table of the HIP kernels (see invertavatar_amd/mc_table.py).

Usage: python tools/gen_mc_tables.py  (tests/test_geometry_cpu.py regenerates it and compares byte for byte)."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from invertavatar_amd import mc_table  # noqa: E402

OUT = os.path.join(REPO, 'invertavatar_amd', 'csrc', 'mc_tables.h')

if __name__ == '__main__':
    with open(OUT, 'w') as fh:
        fh.write(mc_table.header_text())
    count, _, max_tris = mc_table.tables()
    print(f'wrote {OUT}: {int(count.sum())} triangles over 256 cases, at most {max_tris} per case')
