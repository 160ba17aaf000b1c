"""Records tests/golden/desc_one_launch/pool_exhaustion.npz: the flags, neighbour counts and descriptor rows of the
pool-exhaustion scene of tests/test_gpu_desc_one_launch.py, as a given build of the library produces them.
  python tools/record_pool_exhaustion.py libfx_hip_parent.so OUT.npz     (a library under feature_extraction_amd/lib)
The committed file was recorded from the library built at the commit before the descriptor tiers shared a launch."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from feature_extraction_amd import capi  # noqa: E402

capi.LIB_PATH = os.path.join(os.path.dirname(capi.LIB_PATH), sys.argv[1])
from tests import test_gpu_desc_one_launch as t  # noqa: E402

got, _ = t.run_exhaustion()
np.savez(sys.argv[2], flags=np.uint32(got["flags"]), kp_neighbors=np.array(got["kp_neighbors"], np.uint32),
         descriptors=np.array(got["descriptors"], np.float32))
print("flags", hex(got["flags"]), "neighbours", got["kp_neighbors"].tolist(),
      "NaN rows", [k for k in range(got["n_keypoints"]) if np.isnan(got["descriptors"][k, 0])])
