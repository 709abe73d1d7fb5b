"""the reference's coclr_utils package: the tensor clip transforms (transforms.py)"""
from . import transforms  # noqa: F401
