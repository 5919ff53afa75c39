"""Per-scan fusion parameters of the DTU / Tanks&Temples protocols (the reference's tools/gipuma/conf.py values).
nviewss: views of the scan; prob_threshold: depth kept where the confidence reaches it; check_views: agreeing views needed
(fusibile's num_consistent); disp_threshold: disparity agreement bound (fusibile's disp_thresh)."""

DTU_SCANS = [1, 4, 9, 10, 11, 12, 13, 15, 23, 24, 29, 32, 33, 34, 48, 49, 62, 75, 77, 110, 114, 118]
DTU = {"nviewss": 49, "prob_threshold": 0.6, "check_views": 3, "disp_threshold": 0.25}

TANKS_INTERMEDIATE = {
    "Family": {"nviewss": 152, "prob_threshold": 0.8, "check_views": 4, "disp_threshold": 0.25},
    "Francis": {"nviewss": 302, "prob_threshold": 0.6, "check_views": 7, "disp_threshold": 0.2},
    "Horse": {"nviewss": 151, "prob_threshold": 0.6, "check_views": 4, "disp_threshold": 0.25},
    "Lighthouse": {"nviewss": 309, "prob_threshold": 0.6, "check_views": 5, "disp_threshold": 0.3},
    "M60": {"nviewss": 313, "prob_threshold": 0.6, "check_views": 4, "disp_threshold": 0.2},
    "Panther": {"nviewss": 314, "prob_threshold": 0.8, "check_views": 4, "disp_threshold": 0.2},
    "Playground": {"nviewss": 307, "prob_threshold": 0.8, "check_views": 5, "disp_threshold": 0.25},
    "Train": {"nviewss": 301, "prob_threshold": 0.8, "check_views": 5, "disp_threshold": 0.25},
}
TANKS_ADVANCED = {
    "Auditorium": {"nviewss": 302, "prob_threshold": 0.8, "check_views": 3, "disp_threshold": 0.25},
    "Ballroom": {"nviewss": 324, "prob_threshold": 0.8, "check_views": 5, "disp_threshold": 0.25},
    "Courtroom": {"nviewss": 301, "prob_threshold": 0.8, "check_views": 5, "disp_threshold": 0.25},
    "Museum": {"nviewss": 301, "prob_threshold": 0.8, "check_views": 5, "disp_threshold": 0.25},
    "Palace": {"nviewss": 509, "prob_threshold": 0.8, "check_views": 5, "disp_threshold": 0.25},
    "Temple": {"nviewss": 302, "prob_threshold": 0.8, "check_views": 4, "disp_threshold": 0.15},
}


def fusion_args(dataset, scan):
    """dataset: dtu | tanks_intermediate | tanks_advanced; scan: 'scan11' or a Tanks scene name."""
    if dataset == "dtu":
        return dict(DTU)
    table = {"tanks_intermediate": TANKS_INTERMEDIATE, "tanks_advanced": TANKS_ADVANCED}[dataset]
    return dict(table[scan])
