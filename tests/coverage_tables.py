"""Which GPU case covers each source site of a kind; tests/test_host.py keeps both tables in step with csrc/."""

#: every ``gauss_noise(`` call under csrc/: (file, kernel, the case of tests/test_gpu_noise.py that asserts it ran that kernel)
NOISE_SITES = [
    ("rm_kernels.h", "rm_fan_kernel", "test_noise_rm_chunk_and_rays_kernels; test_gpu_parity schedules variant 0"),
    ("rm_kernels.h", "rm_rays_kernel", "test_noise_many_rays_entry_points (RMGPU variant 0)"),
    ("rm_kernels.h", "rm_fan_stream_kernel (2-3 slots)", "test_gpu_parity::test_every_kernel_schedule_is_bit_identical slots 2/3"),
    ("rm_kernels.h", "rm_fan_stream_kernel (1 slot)", "test_gpu_parity schedules variant 1; test_noise_literal_kernels"),
    ("rm_kernels.h", "rm_leftover_kernel", "test_gpu_parity schedules handoff; test_noise_consumers_of_noisy_ranges"),
    ("bl_kernels.h", "bl_fan_kernel", "test_noise_bresenham_kernels (bl_lds, mrx 300 / 700)"),
    ("bl_kernels.h", "occ_fan_lds_kernel", "test_noise_bresenham_kernels (occ_lds)"),
    ("bl_kernels.h", "bl_fan_stream_kernel", "test_noise_bresenham_kernels (bl_stream)"),
    ("bl_kernels.h", "bl_rays_kernel", "test_noise_many_rays_entry_points (Bresenham)"),
    ("lut_kernels.h", "lut_fan_kernel", "test_noise_giant_lut_kernels (lut_fan)"),
    ("lut_kernels.h", "lut_fan_lds_kernel (general statement)", "test_noise_giant_lut_kernels (lut_lds)"),
    ("lut_kernels.h", "lut_rays_kernel", "test_noise_many_rays_entry_points (GiantLUT)"),
    ("cddt_kernels.h", "cddt_fan_bins_kernel", "test_noise_cddt_kernels (cddt_bins, cddt_sort 0 / 1)"),
    ("cddt_kernels.h", "cddt_theta_fan_group", "test_noise_cddt_kernels (cddt_theta, aligned / +4 B output)"),
    ("cddt_kernels.h", "cddt_fan_kernel", "test_noise_cddt_kernels (cddt_rays)"),
    ("cddt_kernels.h", "cddt_rays_kernel", "test_noise_many_rays_entry_points (CDDT)"),
    ("literal_kernels.h", "rm_literal_kernel", "test_noise_literal_kernels; test_noise_many_rays_entry_points (variant 3)"),
]

#: (source file, the freshness test asked, the table it guards, the case that fails when the answer goes stale)
TABLE_CACHES = [
    ("abi_fan.hip", "lut.cache.fresh_for", "ensure_lut: GiantLUT table", "test_warm_handles_follow_a_mutation_script (LUT)"),
    ("abi_fan.hip", "cddt.cache.fresh_for", "ensure_cddt: CDDT blocked table",
     "test_warm_handles_follow_a_mutation_script (CDDT pose-major, theta-major, lds_sort 128); test_multi_device_map_mutations"),
    ("abi_fan.hip", "blpad.cache.fresh_for", "ensure_blpad: Bresenham padded bit maps",
     "test_warm_handles_follow_a_mutation_script (BL variant 1)"),
    ("abi_fan.hip", "step.code_entries_for", "opts_of: code_entries the planner sees",
     "test_code_map_palette_follows_updates"),
    ("abi_fan.hip", "step.fresh_for", "ensure_step_map: step map, code map and palette",
     "test_warm_handles_follow_a_mutation_script (RM, RMGPU code map / row-major); test_entry_points_after_a_stamp"),
    ("abi_fan.hip", "cache.fresh_for", "StepMap::fresh_for: the epoch third of the step map's one test, behind the two rows above",
     "test_warm_handles_follow_a_mutation_script (RM, RMGPU code map / row-major); test_code_map_palette_follows_updates"),
]
