"""tools/tanks_eval: Tanks and Temples F-score evaluation (training scenes, offline protocol) on the GPU."""
