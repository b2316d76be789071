// The driver's option parser as a program of its own (tests/test_host_driver_options.py): main.cpp is included whole, its main()
// renamed, and this main() runs what the driver runs before it touches a file or a device: parse_arguments, then
// check_combinations.  It prints every field of the resulting Config, one name=value per line, and returns the status the driver
// would exit with at that point.  Links like the driver (build/multi_gpu.o, -lmgcfd_hip); needs no GPU.
#define main driver_main
#include "main.cpp"
#undef main

namespace {

void dump(const char *name, const std::string &v) { std::printf("%s=%s\n", name, v.c_str()); }
void dump(const char *name, bool v) { std::printf("%s=%d\n", name, v ? 1 : 0); }
void dump(const char *name, int v) { std::printf("%s=%d\n", name, v); }
void dump(const char *name, size_t v) { std::printf("%s=%zu\n", name, v); }
void dump(const char *name, double v) { std::printf("%s=%.17g\n", name, v); }
void dump(const char *name, const std::vector<int> &v)
{
    std::printf("%s=", name);
    for (size_t k = 0; k < v.size(); k++) std::printf("%s%d", k ? "," : "", v[k]);
    std::printf("\n");
}

#define DUMP(field) dump(#field, c.field)

void dump_config(const Config &c)
{
    DUMP(config_filepath); DUMP(input_file); DUMP(input_file_directory); DUMP(papi_config_file); DUMP(output_file_prefix);
    DUMP(mesh_duplicate_count); DUMP(num_cycles); DUMP(validate_result);
    DUMP(output_variables); DUMP(output_old_variables); DUMP(output_step_factors); DUMP(output_edge_fluxes); DUMP(output_fluxes); DUMP(output_volumes);
    DUMP(timers); DUMP(loop_timers); DUMP(fast_math); DUMP(indirect_rw); DUMP(legacy_ordering);
    DUMP(device); DUMP(gpus); DUMP(gpus_share_device); DUMP(gpus_partition);
    DUMP(output_loads);
    std::printf("loads_ref=%.17g,%.17g,%.17g,%.17g,%.17g\n", c.loads_ref[0], c.loads_ref[1], c.loads_ref[2], c.loads_ref[3], c.loads_ref[4]);
    DUMP(free_stream_given); DUMP(ff_mach); DUMP(angle_of_attack);
    DUMP(polar); DUMP(polar_a0); DUMP(polar_a1); DUMP(polar_n);
    DUMP(time_step_given); DUMP(time_step_mode); DUMP(cfl); DUMP(config_bad);
    DUMP(smoothing_given); DUMP(smoothing_iterations_given); DUMP(smoothing_eps); DUMP(smoothing_iterations);
    DUMP(jst_given); DUMP(jst_kappa2); DUMP(jst_kappa4); DUMP(jst_levels);
    DUMP(upwind_given); DUMP(upwind_levels); DUMP(muscl_levels_said); DUMP(limiter); DUMP(venkat_k); DUMP(entropy_fix);
    DUMP(viscosity_given); DUMP(reynolds_given); DUMP(viscous_extras_given);
    DUMP(viscosity); DUMP(reynolds); DUMP(ref_length); DUMP(prandtl); DUMP(viscous_cfl); DUMP(no_slip); DUMP(viscous_levels);
    DUMP(sutherland); DUMP(smagorinsky); DUMP(model_extras_given);
    DUMP(sutherland_tref); DUMP(sutherland_s); DUMP(smagorinsky_cs); DUMP(prandtl_turbulent);
    DUMP(spalart_allmaras); DUMP(sa_ratio); DUMP(sa_time_accurate); DUMP(sa_unsteady_given); DUMP(sa_length); DUMP(sa_cdes);
    DUMP(wall_damping); DUMP(wall_kappa); DUMP(loads_friction); DUMP(output_surface);
    DUMP(wall_thermal_flags); DUMP(wall_mode); DUMP(wall_value); DUMP(wall_ratio);
    DUMP(face_gradient); DUMP(face_gradient_given); DUMP(viscous_cfl_given); DUMP(loads_heat);
    DUMP(fas); DUMP(cycle_shape); DUMP(pre_sweeps); DUMP(post_sweeps); DUMP(fmg_cycles);
    DUMP(dual_given); DUMP(dual_extras_given); DUMP(dual_dt); DUMP(dual_clamp); DUMP(time_steps); DUMP(bdf_order);
    DUMP(output_statistics); DUMP(statistics_start_given); DUMP(statistics_start);
    DUMP(muscl_levels()); DUMP(loads_width()); DUMP(steps()); DUMP(total_cycles()); DUMP(loads_rows()); DUMP(num_angles());
    dump("angle(0)", c.angle(0));
    dump("angle(num_angles()-1)", c.angle(c.num_angles() - 1));
}

} // namespace

int main(int argc, char **argv)
{
    Config c;
    const bool ok = parse_arguments(argc, argv, c) && check_combinations(c);
    dump_config(c);
    return ok ? 0 : 1;
}
