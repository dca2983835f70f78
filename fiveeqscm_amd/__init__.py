"""fiveeqscm_amd — MI355X-native ensemble engine for the five-equation FaIR model.

Hot path: Python host (torch-ROCm tensors) -> C ABI (include/fiveeq.h) -> one
hand-written HIP kernel per timestep on gfx950.  No CPU fallback for the engine.
"""
from .concentrations import calculate_hfc_conc  # noqa: F401  (reference-compatible, NumPy)
from .minor_gases import minor_gas_rows, minor_gas_rows_host  # noqa: F401  (torch and the library only when the device form is called)
from .aerosols import aerosol_rows, aerosol_rows_host, aci_scale_for_target, aci_scale_for_target_host  # noqa: F401  (likewise)
from .sea_level import SeaLevelComponents, SeaLevelRows, sea_level_rows, sea_level_rows_host  # noqa: F401  (likewise)

__all__ = ["calculate_hfc_conc", "ConcentrationDrivenEngine", "MixedDriveEngine", "minor_gas_rows", "minor_gas_rows_host",
           "aerosol_rows", "aerosol_rows_host", "aci_scale_for_target", "aci_scale_for_target_host",
           "SeaLevelComponents", "SeaLevelRows", "sea_level_rows", "sea_level_rows_host"]
__version__ = "0.1.0"


def __getattr__(name):
    # the engine classes need torch and the built HIP library: imported when first asked for, not with the package
    if name in ("ConcentrationDrivenEngine", "EnsembleEngine", "MixedDriveEngine"):
        from . import engine
        return getattr(engine, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
