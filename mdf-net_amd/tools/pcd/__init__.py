"""tools/pcd: point-cloud fusion with visibility and small-segment filters."""
