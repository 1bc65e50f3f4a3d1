"""MI355X-native BEV-fusion detector hot path (gfx950 HIP kernels behind the reference's module API)."""
__version__ = "0.1.0"

_MAP_TARGETS = ("MapShapes", "pack_shapes", "rasterize", "rasterize_for")
_SWEEPS = ("SweepMerger", "merge_sweeps", "pack_sweeps", "sweep_transforms", "time_lags")
_LAZY = {"map_targets": _MAP_TARGETS, "sweeps": _SWEEPS}
__all__ = ["map_targets", *_MAP_TARGETS, "sweeps", *_SWEEPS]


def __getattr__(name):
    """`map_targets`, `sweeps` and their public names, imported on first use (importing the package stays free of torch)."""
    for module, names in _LAZY.items():
        if name == module or name in names:
            from importlib import import_module
            mod = import_module("." + module, __name__)
            return mod if name == module else getattr(mod, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
