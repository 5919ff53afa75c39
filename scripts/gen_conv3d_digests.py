"""Write tests/golden/conv3d_digests.json: the digests tests/test_conv3d_digests_gpu.py compares against, taken with a library built
from the commit they pin (on an MI355X; scripts/build_variant.sh NAME conv3d.hip, run in a checkout of that commit, builds one):

    MDF_HIP_LIB=/path/to/that/commit's/libmdfnet_hip.so python scripts/gen_conv3d_digests.py COMMIT [OUT.json]

The inputs, the route pins and the digest format are the test module's own functions, so the file and the test cannot drift apart."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mdf-net_amd"), os.path.join(ROOT, "tests")]

import mdfnet_hip  # noqa: E402
import test_conv3d_digests_gpu as T  # noqa: E402

if __name__ == "__main__":
    out = sys.argv[2] if len(sys.argv) > 2 else T.DIGESTS
    doc = {"commit": sys.argv[1], **T.all_digests()}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("library", mdfnet_hip.LIB_PATH, "->", out, ":", sum(len(v) for v in doc["outputs"].values()), "output digests,",
          len(doc["packs"]), "packed sets")
