"""MI355X-native hot path of Medical-SAM2 (per-slice SAM2 forward) -- package root.

Layout:
  csrc/        hand-written HIP kernels (gfx950) + the C-ABI (`include/msam2_hip.h`) -> libmsam2_hip.so
  _lib.py      ctypes loader for the C-ABI library (fails loudly when the library is missing)
  ops.py       thin Python wrappers: torch tensors -> raw pointers/sizes -> C-ABI
  modeling/    host-side mirror of the reference's module interface (same class names, ctor arguments, state-dict
               keys and forward signatures as sam2_train/modeling/**), every forward routed through ops.py
  weights.py   state-dict contract + deterministic name-keyed initialiser
  instances.py instance scores (PQ, AJI, lesion-wise F1) from device-side pair tables (csrc/instances.hip)
  synthetic.py seeded synthetic images / volumes / prompts (BASELINE.json configs)
"""
__version__ = "0.1.0"

# instance scores (instances.py, volume_labels.lesion_scores): resolved on first use, so importing the package loads neither torch nor
# the library
_INSTANCE_NAMES = ("remap_instances", "instances_from_labels", "paint_instances", "instance_tables", "instance_scores_from_tables",
                   "instance_scores")
__all__ = list(_INSTANCE_NAMES) + ["lesion_scores"]


def __getattr__(name):
    if name in _INSTANCE_NAMES:
        from . import instances
        return getattr(instances, name)
    if name == "lesion_scores":
        from .volume_labels import lesion_scores
        return lesion_scores
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
