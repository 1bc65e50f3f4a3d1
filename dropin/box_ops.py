"""Drop-in shim: `import box_ops` resolves to the MI355X-native box geometry module (rotated IoU, box NMS; no counterpart in the
reference).  See INTEGRATION.md."""
import os as _os
import sys as _sys

_sys.path.insert(0, _os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))))
from bevfusion_multimodal_3d_object_detection_amd.box_ops import *  # noqa: F401,F403,E402
