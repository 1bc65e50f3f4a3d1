"""MI355X-native BEV-fusion detector hot path (gfx950 HIP kernels behind the reference's module API)."""
__version__ = "0.1.0"

_MAP_TARGETS = ("MapShapes", "pack_shapes", "rasterize", "rasterize_for")
__all__ = ["map_targets", *_MAP_TARGETS]


def __getattr__(name):
    """`map_targets` and its public names, imported on first use (importing the package stays free of torch)."""
    if name == "map_targets" or name in _MAP_TARGETS:
        from importlib import import_module
        mod = import_module(".map_targets", __name__)
        return mod if name == "map_targets" else getattr(mod, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
