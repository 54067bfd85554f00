"""davo_amd — MI355X-native frame-to-frame pose inference path of DAVO."""
from .launch import bind_rank_cpus as _bind_rank_cpus      # imports os and the standard library only
_bind_rank_cpus()        # a rank started by davo_amd.launch binds itself to its CPU slice before numpy or HIP start a thread
from .version import parse_version, FLAGSHIP_VERSION, VariantConfig, UnsupportedVariantError  # noqa: F401
from .labels import labels_to_u8  # noqa: F401
from .flow import flow_from_f16, flow_to_f16  # noqa: F401
from .depth import depth_from_f16, depth_to_f16  # noqa: F401
from .frames import windows_from_frames, frames_from_windows, frames_plan, flip_windows, flip_frames  # noqa: F401
from .frames import track_pushes, track_pushes_from_windows, track_plan, track_ring  # noqa: F401
from .davo import DAVO, Engine, DavoError, DavoRangeError, conv2d_same, pinned_empty, pin_array, unpin_array  # noqa: F401
from .track import Tracker  # noqa: F401
