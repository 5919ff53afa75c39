"""Point-cloud fusion with normals and voxel downsampling (the reference's tools/pcd/fusion.py with its own defaults).

The same pipeline, parser and scan loop as tools/pcd/fusion.py (build_parser, run, get_cloud), without that file's guard: normals
are estimated unless --no_normal is given (ops.estimate_normals, 30 neighbours, oriented towards the camera) and
--downsample D, or --downsample -1 for the 90th percentile of the nearest-neighbour spacing, replaces the points by the means
of a voxel grid.  The PLY carries nx, ny, nz after z when normals were estimated (read it back with read_ply_normals).

  python mdf-net_amd/tools/pcd/cloud.py -r DATA_ROOT -e OUTPUTS -o PLY_DIR -d tanks -s intermediate [--no_normal] [--downsample -1]
"""
import os
import sys

_TOP = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))     # mdf-net_amd/
if _TOP not in sys.path:
    sys.path.insert(0, _TOP)

from tools.pcd import fusion  # noqa: E402

build_parser = fusion.build_parser


def main(argv=None):
    return fusion.run(build_parser().parse_args(argv))


if __name__ == "__main__":
    main()
