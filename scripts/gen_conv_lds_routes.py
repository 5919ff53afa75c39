"""Write tests/golden/conv_lds_routes.json: the routes, plans and digests tests/test_conv_lds_routes_gpu.py compares against, taken with a
library built from the commit they pin (on an MI355X; scripts/build_variant.sh NAME conv_lds.hip, run in a checkout of that commit,
builds one):

    MDF_HIP_LIB=/path/to/that/commit's/libmdfnet_hip.so python scripts/gen_conv_lds_routes.py COMMIT [OUT.json]

The cases, inputs, switch settings and the record format are the test module's own functions (its child processes inherit MDF_HIP_LIB),
so the file and the test cannot drift apart."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mdf-net_amd"), os.path.join(ROOT, "tests")]

import mdfnet_hip  # noqa: E402
import test_conv_lds_routes_gpu as T  # noqa: E402

if __name__ == "__main__":
    out = sys.argv[2] if len(sys.argv) > 2 else T.GOLDEN
    doc = {"commit": sys.argv[1], "settings": T.all_records()}
    with open(out, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print("library", mdfnet_hip.LIB_PATH, "->", out, ":", {s: len(r) for s, r in doc["settings"].items()}, "cases")
