"""tools/colmap: scene import from a COLMAP sparse model (view selection and depth ranges on the GPU)."""
