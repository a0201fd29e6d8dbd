"""Multi-object tracking behind the detector (reference: ultralytics/trackers)."""
from .bytetrack import ByteTracker, DeviceByteTracker, load_tracker_cfg

__all__ = ["ByteTracker", "DeviceByteTracker", "load_tracker_cfg"]
