"""tools/mesh: TSDF fusion of the filtered depth maps and marching tetrahedra -> a coloured triangle mesh."""
