"""Write tests/golden/wgrad_digests.json: the plans and slab digests tests/test_wgrad_digests_gpu.py compares against, taken with a
library built from the commit they pin (on an MI355X; a checkout of that commit builds one with `python -m mdfnet_hip.build`):

    MDF_HIP_LIB=/path/to/that/commit's/libmdfnet_hip.so python scripts/gen_wgrad_digests.py COMMIT [OUT.json]

The cases, the inputs, the child processes and the digest format are the test module's own functions, so the file and the test
cannot drift apart.  The child processes inherit MDF_HIP_LIB."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mdf-net_amd"), os.path.join(ROOT, "tests")]

import mdfnet_hip  # noqa: E402
import test_wgrad_digests_gpu as T  # noqa: E402

if __name__ == "__main__":
    out = sys.argv[2] if len(sys.argv) > 2 else T.DIGESTS
    doc = {"commit": sys.argv[1], **T.all_digests()}
    with open(out, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print("library", mdfnet_hip.LIB_PATH, "->", out, ":", {k: len(v) for k, v in doc.items() if k != "commit"})
