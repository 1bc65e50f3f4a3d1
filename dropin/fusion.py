"""Drop-in shim: `import fusion` resolves to the MI355X-native module (put this directory on PYTHONPATH
in place of the reference's src/).  See INTEGRATION.md -- also for the keywords beyond the reference's, such as the per-frame
camera calibration `model(imgs, pts, radars, camera_calib=[CameraRig.from_info(info) for info in infos])` of the opt-in
`camera_view_transform: project` branch; without them the reference's scripts see what they always saw."""
import os as _os
import sys as _sys

_sys.path.insert(0, _os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))))
from bevfusion_multimodal_3d_object_detection_amd.fusion import *  # noqa: F401,F403,E402
