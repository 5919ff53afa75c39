"""tools/dtu_eval: DTU point-cloud evaluation (accuracy, completeness) on the GPU: the MATLAB scorer restated."""
