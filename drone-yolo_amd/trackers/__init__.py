"""Multi-object tracking behind the detector (reference: ultralytics/trackers): ByteTrack on the host and on the device, for axis-aligned
rows and (``rotated=True``) for the xywhr rows of oriented-box models."""
from .bytetrack import ByteTracker, DeviceByteTracker, load_tracker_cfg

__all__ = ["ByteTracker", "DeviceByteTracker", "load_tracker_cfg"]
