from .specification import CogVideoXDDIMTables, MI355XCogVideoXModelSpecification, MI355XCogVideoXSpecOps  # noqa: F401
from .block import MI355XCogVideoXBlock  # noqa: F401
from .model import CogVideoXTransformerConfig, MI355XCogVideoXTransformer3DModel  # noqa: F401
from .trainer import MI355XCogVideoXSFTStep  # noqa: F401
from .sampler import (COG_DPM_SCHEDULER_CONFIG, COG_SCHEDULER_CONFIG, MI355XCogVideoXLatentSampler, StepNoiseRequired, cog_ddim_tables,  # noqa: F401
                      cog_dpm_coefficients_f64, cog_dpm_step_noise, cog_dpm_tables, cog_guidance_table)
