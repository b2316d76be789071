// euler3d_gpu_double — drop-in replacement for the reference's euler3d_cpu_double binary
// (src/euler3d_cpu_double.cpp) on one MI355X, written purely against the C ABI of
// include/mgcfd.h.  Same command line (src/Base/config.cpp:32-47), same input.dat / mesh /
// .coords / MG-map inputs, same stdout progress lines, same `variables` dump, and the same
// Times.csv / LoopNumIters.csv schema (src/Monitoring/timer.cpp:106-195,
// src/Monitoring/loop_stats.cpp:83-171, identification columns src/Base/io_enhanced.cpp:858-1016).
#include <getopt.h>
#include <sched.h>
#include <unistd.h>

#include <cctype>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <numeric>
#include <sstream>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "mgcfd.h"
#include "multi_gpu.hpp"

namespace {

struct Config {                       // the reference's `config` (src/Base/config.h:27-47)
    std::string config_filepath, input_file, input_file_directory, papi_config_file, output_file_prefix;
    int mesh_duplicate_count = 1;
    int num_cycles = 25;              // src/Base/config.cpp:63
    bool validate_result = false;
    bool output_variables = false, output_old_variables = false, output_step_factors = false,
         output_edge_fluxes = false, output_fluxes = false, output_volumes = false;
    // extensions (not in the reference)
    bool timers = true;               // --no-timers: fused fast path (one launch per Runge-Kutta stage); Times.csv holds only Total
    bool loop_timers = false;         // --loop-timers: EVERY loop its own launch between two events, as the reference's -DTIME build brackets
                                      // them (src/Monitoring/timer.cpp:58-195); default: fused stages, the per-loop times ATTRIBUTED
                                      // from every 32nd sweep / transfer of a level, which runs per loop under events (MGCFD_OPT_TIMING = 4)
    bool fast_math = false;           // --fast: allow FMA contraction (MGCFD_OPT_EXACT = 0)
    bool indirect_rw = true;          // the reference runs the probe every RK stage; --no-indirect-rw skips it
    bool legacy_ordering = false;     // --legacy-ordering: the reference's -DLEGACY_ORDERING edge sort (a compile-time flag there)
    int device = 0;
    int gpus = 1;                     // --gpus N: a single-level input partitioned over N GPUs, a multigrid input one level per GPU
    bool gpus_share_device = false;   // --gpus-share-device: all N ranks on --device (rehearsal on a one-GPU box)
    bool gpus_partition = false;      // --gpus-partition: split every level of a multigrid input over the N GPUs (the default when N > levels)
    bool output_loads = false;        // --output-loads: the level-0 surface loads of every cycle into surface_loads.* (one GPU, or --gpus N --gpus-partition)
    double loads_ref[5] = {1.0, 1.0, 0.0, 0.0, 0.0};   // --loads-reference=S,c,x,y,z: reference area, length and moment point
    // the free stream (the reference compiles it in: ff_mach = 1.2, deg_angle_of_attack = 0, src/Base/const.h:14-15)
    bool free_stream_given = false;   // --mach / --alpha / ff_mach / angle_of_attack: mgcfd_set_free_stream before the first cycle
    double ff_mach = 1.2, angle_of_attack = 0.0;
    bool polar = false;               // --polar A0:A1:N: N angles from A0 to A1 inclusive, -g cycles each, polar.csv
    double polar_a0 = 0.0, polar_a1 = 0.0;
    int polar_n = 0;
    // the time step (the reference ties it to the mesh name and the literal 0.5, src/euler3d_cpu_double.cpp:388-395)
    bool time_step_given = false;     // --time-step / --cfl / time_step / cfl: mgcfd_set_time_step before the first cycle
    int time_step_mode = MGCFD_DT_REFERENCE;
    double cfl = 0.5;
    bool config_bad = false;          // a config file's value (time step, residual smoothing) was refused: the run ends right after parsing
    // implicit residual smoothing: --residual-smoothing EPS / --smoothing-iterations N / residual_smoothing / smoothing_iterations
    bool smoothing_given = false;     // an EPS was given: mgcfd_set_residual_smoothing before the first cycle
    bool smoothing_iterations_given = false;
    double smoothing_eps = 0.0;
    int smoothing_iterations = 2;     // (the default when only EPS is given)
    // JST dissipation: --jst / --jst-kappa2 X / --jst-kappa4 X / --jst-levels N and the config keys jst (Y) / jst_kappa2 / jst_kappa4 /
    // jst_levels; each of the three values implies --jst
    bool jst_given = false;           // mgcfd_set_jst before the first cycle
    double jst_kappa2 = MGCFD_JST_KAPPA2, jst_kappa4 = MGCFD_JST_KAPPA4;
    int jst_levels = 1;
    // upwind fluxes: --upwind / --upwind-levels N / --muscl-levels N / --limiter NAME / --venkat-k X / --entropy-fix X and the config
    // keys upwind (Y) / upwind_levels / muscl_levels / limiter / venkat_k / entropy_fix; each of the five values implies --upwind
    bool upwind_given = false;        // mgcfd_set_upwind before the first cycle
    int upwind_levels = 1, muscl_levels_said = -1, limiter = MGCFD_LIMITER_VENKATAKRISHNAN;
    double venkat_k = MGCFD_UPWIND_VENKAT_K, entropy_fix = MGCFD_UPWIND_ENTROPY_FIX;
    int muscl_levels() const { return muscl_levels_said < 0 ? upwind_levels : muscl_levels_said; }   // (not said: every upwind level reconstructs)
    // laminar viscous terms: --viscosity MU or --reynolds RE (with --ref-length L), --prandtl X, --no-slip, --viscous-cfl X,
    // --viscous-levels N and the config keys viscosity / reynolds / ref_length / prandtl / no_slip (Y) / viscous_cfl / viscous_levels
    bool viscosity_given = false, reynolds_given = false;   // one of the two switches the terms on: mgcfd_set_viscous before the first cycle
    bool viscous_extras_given = false;                      // one of the companions was given (they need MU or RE)
    double viscosity = 0.0, reynolds = 0.0, ref_length = 1.0, prandtl = MGCFD_VISCOUS_PRANDTL, viscous_cfl = MGCFD_VISCOUS_CFL;
    bool no_slip = false;
    int viscous_levels = 1;
    bool viscous() const { return viscosity_given || reynolds_given; }
    // the viscosity model: --sutherland with --sutherland-tref X and --sutherland-s X, --smagorinsky [CS], --prandtl-turbulent X and
    // the config keys sutherland (Y) / sutherland_tref / sutherland_s / smagorinsky (Y or CS) / prandtl_turbulent
    bool sutherland = false, smagorinsky = false;
    bool model_extras_given = false;                        // --sutherland-tref / --sutherland-s / --prandtl-turbulent
    double sutherland_tref = 0.0, sutherland_s = MGCFD_SUTHERLAND_S, smagorinsky_cs = MGCFD_SMAGORINSKY_CS, prandtl_turbulent = MGCFD_PRANDTL_TURBULENT;
    bool viscosity_model() const { return sutherland || smagorinsky || spalart_allmaras; }
    // --spalart-allmaras[=RATIO] / spalart_allmaras = Y | RATIO: the transported eddy viscosity (MGCFD_EDDY_SPALART_ALLMARAS),
    // RATIO the free-stream nu_tilde over nu (mgcfd_set_sa_free_stream)
    bool spalart_allmaras = false;
    double sa_ratio = MGCFD_SA_RATIO;
    // --sa-time-accurate, --sa-length wall|des|ddes, --sa-cdes X and the config keys sa_time_accurate (Y) / sa_length / sa_cdes:
    // the unsteady model (mgcfd_set_sa_unsteady), with --spalart-allmaras; --sa-time-accurate lets it run with --physical-time-step
    bool sa_time_accurate = false, sa_unsteady_given = false;
    int sa_length = MGCFD_SA_LENGTH_WALL;
    double sa_cdes = MGCFD_SA_CDES;
    // --wall-damping[=KAPPA] / wall_damping = Y | KAPPA: the wall-limited length scale of --smagorinsky (mgcfd_set_wall_damping)
    bool wall_damping = false;
    double wall_kappa = MGCFD_WALL_KAPPA;
    bool loads_friction = false;      // --loads-friction: the friction loads beside the pressure loads in surface_loads.* and polar.csv (one GPU)
    bool output_surface = false;      // --output-surface: Cp and Cf per wall node of level 0 into surface.* (one GPU)
    // wall thermal conditions (mgcfd_set_wall_temperature): --wall-temperature T, --wall-temperature-ratio R (times the static
    // free-stream temperature in use) or --wall-heat-flux Q, with --no-slip and the viscous terms; one of them at most
    int wall_thermal_flags = 0;       // how many of the three were given
    int wall_mode = 0;                // MGCFD_WALL_*
    double wall_value = 0.0;          // T, R or Q as given
    bool wall_ratio = false;          // ... it is R
    // --face-gradient averaged|corrected (config key face_gradient; mgcfd_set_face_gradient): the face gradient of the viscous and
    // Spalart-Allmaras diffusion.  Corrected without --viscous-cfl: MGCFD_VISCOUS_CFL_CORRECTED.  One GPU
    int face_gradient = MGCFD_FACE_GRADIENT_AVERAGED;
    bool face_gradient_given = false, viscous_cfl_given = false;
    bool loads_heat = false;          // --loads-heat: Q, A and the mean Stanton number behind the friction columns; qw, T, St in surface.* (one GPU)
    size_t loads_width() const { return loads_heat ? 14 : (loads_friction ? 12 : 6); }
    // FAS multigrid: --fas and the config key fas (Y): mgcfd_set_fas before the first cycle; one GPU, two levels or more
    bool fas = false;
    // the multigrid cycle: --cycle V|W|F, --pre-sweeps LIST, --post-sweeps LIST (mgcfd_set_cycle before the first cycle) and
    // --fmg-cycles LIST (mgcfd_full_multigrid before the -g cycles); the lists are expanded once the number of levels is known
    int cycle_shape = MGCFD_CYCLE_V;
    std::vector<int> pre_sweeps, post_sweeps, fmg_cycles;
    bool cycle_given() const { return cycle_shape != MGCFD_CYCLE_V || !pre_sweeps.empty() || !post_sweeps.empty(); }
    // dual time stepping: --physical-time-step DT / --time-steps N / --dual-time-clamp X / --bdf-order 1|2 and the config keys
    // physical_time_step / time_steps / dual_time_clamp / bdf_order.  With DT given, -g is the number of cycles per physical step.
    bool dual_given = false;          // a DT was given: mgcfd_set_dual_time before the first cycle, mgcfd_advance for the cycles
    bool dual_extras_given = false;   // one of the three companions was given (they need DT)
    double dual_dt = 0.0, dual_clamp = MGCFD_DUAL_TIME_CLAMP;
    int time_steps = 1, bdf_order = 2;
    // flow statistics (mgcfd_set_statistics): --output-statistics writes statistics.* (and, with --output-surface,
    // surface_statistics.*) from the samples mgcfd_advance takes; --statistics-start K: the first K physical steps are not sampled.
    // Dual-time runs on one GPU only.
    bool output_statistics = false, statistics_start_given = false;
    int statistics_start = 0;
    int steps() const { return dual_given ? time_steps : 1; }
    int total_cycles() const { return (num_cycles > 0 ? num_cycles : 0) * steps(); }      // RMS lines of the run
    int loads_rows() const { return dual_given ? time_steps : (num_cycles > 0 ? num_cycles : 0); }   // one row per physical step
    // the k-th angle of the run (one angle without --polar)
    int num_angles() const { return polar ? polar_n : 1; }
    double angle(int k) const { return !polar ? angle_of_attack : (polar_n == 1 ? polar_a0 : polar_a0 + (polar_a1 - polar_a0) * double(k) / double(polar_n - 1)); }
};

// one finite number and nothing else
bool parse_number(const char *text, double *out)
{
    if (!text || *text == '\0' || std::isspace(static_cast<unsigned char>(*text))) return false;
    char *end = nullptr;
    const double v = std::strtod(text, &end);
    if (end == text || *end != '\0' || !std::isfinite(v)) return false;
    *out = v;
    return true;
}

// reference | global | local | local-legacy (or local_legacy)
bool parse_time_step_mode(const char *text, int *out)
{
    const std::string t(text ? text : "");
    if (t == "reference") *out = MGCFD_DT_REFERENCE;
    else if (t == "global") *out = MGCFD_DT_GLOBAL;
    else if (t == "local") *out = MGCFD_DT_LOCAL;
    else if (t == "local-legacy" || t == "local_legacy") *out = MGCFD_DT_LOCAL_LEGACY;
    else return false;
    return true;
}
// a finite number above zero (the CFL number, the residual smoothing's coefficient)
bool parse_positive(const char *text, double *out)
{
    double v = 0.0;
    if (!parse_number(text, &v) || !(v > 0.0)) return false;
    *out = v;
    return true;
}

// --limiter / limiter: "none", "barth-jespersen" or "venkatakrishnan"
bool set_limiter(Config &c, const char *text)
{
    const std::string v(text);
    if (v == "none") c.limiter = MGCFD_LIMITER_NONE;
    else if (v == "barth-jespersen") c.limiter = MGCFD_LIMITER_BARTH_JESPERSEN;
    else if (v == "venkatakrishnan") c.limiter = MGCFD_LIMITER_VENKATAKRISHNAN;
    else return false;
    c.upwind_given = true;
    return true;
}
// --face-gradient / face_gradient: "averaged" or "corrected"
bool set_face_gradient(Config &c, const char *text)
{
    const std::string v(text ? text : "");
    if (v != "averaged" && v != "corrected") return false;
    c.face_gradient = v == "corrected" ? MGCFD_FACE_GRADIENT_CORRECTED : MGCFD_FACE_GRADIENT_AVERAGED;
    c.face_gradient_given = true;
    return true;
}
// --sa-length / sa_length: the model length of the Spalart-Allmaras model by name
bool set_sa_length(Config &c, const char *text)
{
    const std::string v(text ? text : "");
    if (v != "wall" && v != "des" && v != "ddes") return false;
    c.sa_length = v == "ddes" ? MGCFD_SA_LENGTH_DDES : (v == "des" ? MGCFD_SA_LENGTH_DES : MGCFD_SA_LENGTH_WALL);
    return true;
}

// one of the three wall thermal settings: which = 0 --wall-temperature T, 1 --wall-temperature-ratio R (both above zero),
// 2 --wall-heat-flux Q (any finite number); counts how many were given
bool set_wall_thermal(Config &c, int which, const char *text)
{
    double v = 0.0;
    if (which == 2 ? !parse_number(text, &v) : !parse_positive(text, &v)) return false;
    c.wall_thermal_flags++;
    c.wall_mode = which == 2 ? MGCFD_WALL_HEAT_FLUX : MGCFD_WALL_ISOTHERMAL;
    c.wall_value = v;
    c.wall_ratio = which == 1;
    return true;
}

// the smoothing's Jacobi iterations: a whole number 0 ... MGCFD_MAX_SMOOTHING_ITERATIONS
bool parse_smoothing_iterations(const char *text, int *out)
{
    double v = 0.0;
    if (!parse_number(text, &v) || v < 0.0 || v > double(MGCFD_MAX_SMOOTHING_ITERATIONS) || v != double(int(v))) return false;
    *out = int(v);
    return true;
}

// a finite number not below zero (the JST coefficients)
bool parse_not_negative(const char *text, double *out)
{
    double v = 0.0;
    if (!parse_number(text, &v) || !(v >= 0.0)) return false;
    *out = v;
    return true;
}

// a whole number lo ... hi (the physical time steps, the BDF order, the JST levels)
bool parse_whole(const char *text, int lo, int hi, int *out)
{
    double v = 0.0;
    if (!parse_number(text, &v) || v < double(lo) || v > double(hi) || v != double(int(v))) return false;
    *out = int(v);
    return true;
}
// "N" or "N,N,...": whole numbers lo ... hi (the sweeps per level, the FMG cycles per level)
bool parse_whole_list(const char *text, int lo, int hi, std::vector<int> *out)
{
    out->clear();
    const std::string all(text);
    for (size_t at = 0; at <= all.size();) {
        const size_t comma = std::min(all.find(',', at), all.size());
        int v = 0;
        if (!parse_whole(all.substr(at, comma - at).c_str(), lo, hi, &v)) return false;
        out->push_back(v);
        at = comma + 1;
    }
    return !out->empty();
}
constexpr int kMaxTimeSteps = 1000000;
constexpr int kMaxJstLevels = 64;

// "A0:A1:N": two finite angles and a count of at least 1
bool parse_polar(const char *text, Config &c)
{
    const std::string t(text ? text : "");
    const size_t p1 = t.find(':'), p2 = p1 == std::string::npos ? p1 : t.find(':', p1 + 1);
    if (p2 == std::string::npos || t.find(':', p2 + 1) != std::string::npos) return false;
    double n = 0.0;
    if (!parse_number(t.substr(0, p1).c_str(), &c.polar_a0) || !parse_number(t.substr(p1 + 1, p2 - p1 - 1).c_str(), &c.polar_a1) ||
        !parse_number(t.substr(p2 + 1).c_str(), &n))
        return false;
    if (n < 1.0 || n > 100000.0 || n != std::floor(n)) return false;
    c.polar_n = static_cast<int>(n);
    c.polar = true;
    return true;
}

// "S,c,x,y,z": five finite numbers, S and c positive; false on anything else
bool parse_loads_reference(const char *text, double out[5])
{
    const char *p = text;
    for (int k = 0; k < 5; k++) {
        if (k > 0) {
            if (*p != ',') return false;
            p++;
        }
        if (*p == '\0' || *p == ',' || std::isspace(static_cast<unsigned char>(*p))) return false;
        char *end = nullptr;
        const double v = std::strtod(p, &end);
        if (end == p || !std::isfinite(v)) return false;
        out[k] = v;
        p = end;
    }
    return *p == '\0' && out[0] > 0.0 && out[1] > 0.0;
}

std::string trim(const std::string &s)
{
    size_t b = s.find_first_not_of(" \t\r\n");
    if (b == std::string::npos) return "";
    return s.substr(b, s.find_last_not_of(" \t\r\n") - b + 1);
}

void set_param(Config &c, const std::string &key, const std::string &value)
{
    // src/Base/config.cpp:81-157
    if (key == "config_filepath") c.config_filepath = value;
    else if (key == "input_file") c.input_file = value;
    else if (key == "input_file_directory") c.input_file_directory = value;
    else if (key == "papi_config_file") c.papi_config_file = value;
    else if (key == "output_file_prefix") c.output_file_prefix = value;
    else if (key == "mesh_duplicate_count") c.mesh_duplicate_count = std::atoi(value.c_str());
    else if (key == "cycles") c.num_cycles = std::atoi(value.c_str());
    else if (key == "omp_num_threads") { /* no OpenMP here */ }
    else if (key == "output_variables") { if (value == "Y") c.output_variables = true; }
    else if (key == "output_old_variables") { if (value == "Y") c.output_old_variables = true; }
    else if (key == "output_step_factors") { if (value == "Y") c.output_step_factors = true; }
    else if (key == "output_edge_fluxes") { if (value == "Y") c.output_edge_fluxes = true; }
    else if (key == "output_fluxes") { if (value == "Y") c.output_fluxes = true; }
    else if (key == "output_volumes") { if (value == "Y") c.output_volumes = true; }
    else if (key == "ff_mach") { if (parse_number(value.c_str(), &c.ff_mach)) c.free_stream_given = true; else std::printf("WARNING: ff_mach = '%s' is not a number.\n", value.c_str()); }
    else if (key == "angle_of_attack") { if (parse_number(value.c_str(), &c.angle_of_attack)) c.free_stream_given = true; else std::printf("WARNING: angle_of_attack = '%s' is not a number.\n", value.c_str()); }
    else if (key == "time_step") {
        if (parse_time_step_mode(value.c_str(), &c.time_step_mode)) c.time_step_given = true;
        else { std::fprintf(stderr, "ERROR: time_step = '%s': expected reference, global, local or local-legacy\n", value.c_str()); c.config_bad = true; }
    }
    else if (key == "cfl") {
        if (parse_positive(value.c_str(), &c.cfl)) c.time_step_given = true;
        else { std::fprintf(stderr, "ERROR: cfl = '%s': expected a finite number above zero\n", value.c_str()); c.config_bad = true; }
    }
    else if (key == "residual_smoothing") {
        if (parse_positive(value.c_str(), &c.smoothing_eps)) c.smoothing_given = true;
        else { std::fprintf(stderr, "ERROR: residual_smoothing = '%s': expected a finite number above zero\n", value.c_str()); c.config_bad = true; }
    }
    else if (key == "smoothing_iterations") {
        if (parse_smoothing_iterations(value.c_str(), &c.smoothing_iterations)) c.smoothing_iterations_given = true;
        else { std::fprintf(stderr, "ERROR: smoothing_iterations = '%s': expected a whole number 0 ... %d\n", value.c_str(), MGCFD_MAX_SMOOTHING_ITERATIONS); c.config_bad = true; }
    }
    else if (key == "jst") { if (value == "Y") c.jst_given = true; }
    else if (key == "fas") { if (value == "Y") c.fas = true; }
    else if (key == "jst_kappa2" || key == "jst_kappa4") {
        if (parse_not_negative(value.c_str(), key == "jst_kappa2" ? &c.jst_kappa2 : &c.jst_kappa4)) c.jst_given = true;
        else { std::fprintf(stderr, "ERROR: %s = '%s': expected a finite number, zero or above\n", key.c_str(), value.c_str()); c.config_bad = true; }
    }
    else if (key == "jst_levels") {
        if (parse_whole(value.c_str(), 0, kMaxJstLevels, &c.jst_levels)) c.jst_given = true;
        else { std::fprintf(stderr, "ERROR: jst_levels = '%s': expected a whole number 0 ... %d\n", value.c_str(), kMaxJstLevels); c.config_bad = true; }
    }
    else if (key == "upwind") { if (value == "Y") c.upwind_given = true; }
    else if (key == "upwind_levels" || key == "muscl_levels") {
        if (parse_whole(value.c_str(), 0, kMaxJstLevels, key == "upwind_levels" ? &c.upwind_levels : &c.muscl_levels_said)) c.upwind_given = true;
        else { std::fprintf(stderr, "ERROR: %s = '%s': expected a whole number 0 ... %d\n", key.c_str(), value.c_str(), kMaxJstLevels); c.config_bad = true; }
    }
    else if (key == "limiter") {
        if (!set_limiter(c, value.c_str())) { std::fprintf(stderr, "ERROR: limiter = '%s': expected none, barth-jespersen or venkatakrishnan\n", value.c_str()); c.config_bad = true; }
    }
    else if (key == "venkat_k") {
        if (parse_positive(value.c_str(), &c.venkat_k)) c.upwind_given = true;
        else { std::fprintf(stderr, "ERROR: venkat_k = '%s': expected a finite number above zero\n", value.c_str()); c.config_bad = true; }
    }
    else if (key == "entropy_fix") {
        if (parse_not_negative(value.c_str(), &c.entropy_fix) && c.entropy_fix <= 1.0) c.upwind_given = true;
        else { std::fprintf(stderr, "ERROR: entropy_fix = '%s': expected a number 0 ... 1\n", value.c_str()); c.config_bad = true; }
    }
    else if (key == "viscosity" || key == "reynolds" || key == "ref_length" || key == "prandtl" || key == "viscous_cfl") {
        double *dst = key == "viscosity" ? &c.viscosity : key == "reynolds" ? &c.reynolds : key == "ref_length" ? &c.ref_length : key == "prandtl" ? &c.prandtl : &c.viscous_cfl;
        if (parse_positive(value.c_str(), dst)) {
            if (key == "viscosity") c.viscosity_given = true; else if (key == "reynolds") c.reynolds_given = true; else c.viscous_extras_given = true;
            if (key == "viscous_cfl") c.viscous_cfl_given = true;
        }
        else { std::fprintf(stderr, "ERROR: %s = '%s': expected a finite number above zero\n", key.c_str(), value.c_str()); c.config_bad = true; }
    }
    else if (key == "sutherland") { if (value == "Y") c.sutherland = true; }
    else if (key == "smagorinsky") {
        if (value == "Y") c.smagorinsky = true;
        else if (parse_positive(value.c_str(), &c.smagorinsky_cs)) c.smagorinsky = true;
        else if (value != "N") { std::fprintf(stderr, "ERROR: smagorinsky = '%s': expected Y or a finite constant above zero\n", value.c_str()); c.config_bad = true; }
    }
    else if (key == "spalart_allmaras") {
        if (value == "Y") c.spalart_allmaras = true;
        else if (parse_positive(value.c_str(), &c.sa_ratio)) c.spalart_allmaras = true;
        else if (value != "N") { std::fprintf(stderr, "ERROR: spalart_allmaras = '%s': expected Y or a finite ratio above zero\n", value.c_str()); c.config_bad = true; }
    }
    else if (key == "sa_time_accurate") { if (value == "Y") { c.sa_time_accurate = true; c.sa_unsteady_given = true; } }
    else if (key == "sa_length") {
        if (set_sa_length(c, value.c_str())) c.sa_unsteady_given = true;
        else { std::fprintf(stderr, "ERROR: sa_length = '%s': expected wall, des or ddes\n", value.c_str()); c.config_bad = true; }
    }
    else if (key == "sa_cdes") {
        if (parse_positive(value.c_str(), &c.sa_cdes)) c.sa_unsteady_given = true;
        else { std::fprintf(stderr, "ERROR: sa_cdes = '%s': expected a finite number above zero\n", value.c_str()); c.config_bad = true; }
    }
    else if (key == "wall_damping") {
        if (value == "Y") c.wall_damping = true;
        else if (parse_positive(value.c_str(), &c.wall_kappa)) c.wall_damping = true;
        else if (value != "N") { std::fprintf(stderr, "ERROR: wall_damping = '%s': expected Y or a finite constant above zero\n", value.c_str()); c.config_bad = true; }
    }
    else if (key == "sutherland_tref" || key == "sutherland_s" || key == "prandtl_turbulent") {
        double *dst = key == "sutherland_tref" ? &c.sutherland_tref : key == "sutherland_s" ? &c.sutherland_s : &c.prandtl_turbulent;
        if (parse_positive(value.c_str(), dst)) c.model_extras_given = true;
        else { std::fprintf(stderr, "ERROR: %s = '%s': expected a finite number above zero\n", key.c_str(), value.c_str()); c.config_bad = true; }
    }
    else if (key == "no_slip") { if (value == "Y") { c.no_slip = true; c.viscous_extras_given = true; } }
    else if (key == "wall_temperature" || key == "wall_temperature_ratio" || key == "wall_heat_flux") {
        if (!set_wall_thermal(c, key == "wall_heat_flux" ? 2 : (key == "wall_temperature_ratio" ? 1 : 0), value.c_str())) {
            std::fprintf(stderr, "ERROR: %s = '%s': expected a finite number%s\n", key.c_str(), value.c_str(), key == "wall_heat_flux" ? "" : " above zero");
            c.config_bad = true;
        }
    }
    else if (key == "loads_heat") { if (value == "Y") c.loads_heat = true; }
    else if (key == "face_gradient") {
        if (!set_face_gradient(c, value.c_str())) { std::fprintf(stderr, "ERROR: face_gradient = '%s': expected averaged or corrected\n", value.c_str()); c.config_bad = true; }
    }
    else if (key == "viscous_levels") {
        if (parse_whole(value.c_str(), 0, kMaxJstLevels, &c.viscous_levels)) c.viscous_extras_given = true;
        else { std::fprintf(stderr, "ERROR: viscous_levels = '%s': expected a whole number 0 ... %d\n", value.c_str(), kMaxJstLevels); c.config_bad = true; }
    }
    else if (key == "physical_time_step") {
        if (parse_positive(value.c_str(), &c.dual_dt)) c.dual_given = true;
        else { std::fprintf(stderr, "ERROR: physical_time_step = '%s': expected a finite number above zero\n", value.c_str()); c.config_bad = true; }
    }
    else if (key == "time_steps") {
        if (parse_whole(value.c_str(), 1, kMaxTimeSteps, &c.time_steps)) c.dual_extras_given = true;
        else { std::fprintf(stderr, "ERROR: time_steps = '%s': expected a whole number 1 ... %d\n", value.c_str(), kMaxTimeSteps); c.config_bad = true; }
    }
    else if (key == "dual_time_clamp") {
        if (parse_positive(value.c_str(), &c.dual_clamp)) c.dual_extras_given = true;
        else { std::fprintf(stderr, "ERROR: dual_time_clamp = '%s': expected a finite number above zero\n", value.c_str()); c.config_bad = true; }
    }
    else if (key == "bdf_order") {
        if (parse_whole(value.c_str(), 1, 2, &c.bdf_order)) c.dual_extras_given = true;
        else { std::fprintf(stderr, "ERROR: bdf_order = '%s': expected 1 or 2\n", value.c_str()); c.config_bad = true; }
    }
    else std::printf("WARNING: Unknown key '%s' encountered during parsing of config file.\n", key.c_str());
}

void read_config(Config &c)
{
    // src/Base/config.cpp:159-217
    if (access(c.config_filepath.c_str(), F_OK) == -1) {
        std::fprintf(stderr, "ERROR: \"%s\" does not exist.\n", c.config_filepath.c_str());
        return;
    }
    std::ifstream file(c.config_filepath);
    std::string line;
    while (std::getline(file, line)) {
        if (!line.empty() && line[0] == '#') continue;
        size_t eq = line.find('=');
        if (eq == std::string::npos || eq + 1 >= line.size()) continue;
        set_param(c, trim(line.substr(0, eq)), trim(line.substr(eq + 1)));
    }
    std::string dir;
    size_t slash = c.config_filepath.rfind('/');
    if (slash != std::string::npos) dir = c.config_filepath.substr(0, slash);
    if ((c.input_file_directory.empty() || c.input_file_directory[0] != '/') && !dir.empty()) {
        if (c.input_file_directory == "./") c.input_file_directory = dir;
        else c.input_file_directory = dir + "/" + c.input_file_directory;
    }
}

void print_help()
{
    std::fprintf(stderr,
        "MG-CFD (MI355X) instructions\n\n"
        "Usage: euler3d_gpu_double [OPTIONS] \n\n"
        "  -h, --help                       Print help\n\n"
        "CRITICAL ARGUMENTS\n  One of these must be set:\n"
        "  -i, --input-file=FILEPATH        Multigrid input grid (.dat file)\n"
        "  -c, --config-filepath=FILEPATH   Config file\n\n"
        "OPTIONAL ARGUMENTS\n"
        "  -d, --input-directory=DIRPATH    Directory path to input files\n"
        "  -o, --output-file-prefix=STRING  String to prepend to output filenames\n"
        "  -p, --papi-config-file=FILEPATH  Accepted and ignored (CPU performance counters)\n\n"
        "  -g, --num-cycles=INT             Number of multigrid V-cycles\n"
        "  -m, --mesh-duplicate-count=INT   Number of times to duplicate mesh\n"
        "  -v, --validate-result            Check final state against pre-calculated solution\n\n"
        "DEBUGGING ARGUMENTS\n"
        "  --output-variables               Write Euler equation variable values to file\n"
        "  --output-fluxes                  Write flux accumulations to file\n"
        "  --output-step-factors            Write step factors to file\n\n"
        "GPU ARGUMENTS (extensions)\n"
        "  --device=INT                     GPU to run on (default 0); with --gpus the first of the N devices\n"
        "  --gpus=INT                       Run on N GPUs of this node: a single-level input is partitioned over them\n"
        "                                   (halo messages after every Runge-Kutta stage), a multigrid input runs one\n"
        "                                   level per GPU; fused path (as --no-timers)\n"
        "  --gpus-share-device              With --gpus: every rank on the one device (functional rehearsal)\n"
        "  --gpus-partition                 With --gpus on a multigrid input: split EVERY level over the N GPUs and run the\n"
        "                                   whole V-cycle inside the library (the default when N exceeds the number of levels)\n"
        "  --no-timers                      One fused launch per Runge-Kutta stage; no per-loop times\n"
        "  --loop-timers                    Every loop its own launch between two events (2.7x slower cycles); default: fused\n"
        "                                   stages, per-loop times attributed from every 32nd sweep, which runs per loop\n"
        "  --no-indirect-rw                 Skip the indirect_rw bandwidth probe each RK stage\n"
        "  --fast                           Fast mode: FMA contraction and order-free flux accumulation (results within\n"
        "                                   1e-12 relative of the reference's per sweep, not reproducible bit for bit from run to run)\n"
        "  --legacy-ordering                Sort edges by (a,b,x,y,z) like the reference built with -DLEGACY_ORDERING\n"
        "  --output-loads                   Write the pressure force and moment on the solid walls and their coefficients\n"
        "                                   after every cycle to surface_loads.* (CSV).  One GPU, or --gpus N together\n"
        "                                   with --gpus-partition (every level split over the ranks; the same file, byte\n"
        "                                   for byte); refused with --gpus N alone\n"
        "  --loads-reference=S,c,x,y,z      Reference area, length and moment point of --output-loads (default 1,1,0,0,0)\n"
        "  --mach=M                         Free-stream Mach number (default 1.2, the reference's; config key ff_mach)\n"
        "  --alpha=DEG                      Angle of attack in degrees, inside (-90, 90) (default 0; config key angle_of_attack)\n"
        "  --loads-friction                 With the viscous terms and --output-loads or --polar: the thirteen columns are computed from the\n"
        "                                   total of pressure and friction loads, and the friction loads Fxv ... Mzv and their\n"
        "                                   coefficients CDv ... CMzv follow them.  One GPU\n"
        "  --output-surface                 Write surface.* (CSV): one row per solid-wall node of level 0 in the final state, its\n"
        "                                   coordinates, wall area vector, Cp and the tangential Cf vector.  One GPU\n"
        "  --wall-temperature=T             With --no-slip: the wall is held at temperature T (T = p / rho) instead of adiabatic\n"
        "                                   (config key wall_temperature).  One GPU\n"
        "  --wall-temperature-ratio=R       ... at R times the static free-stream temperature in use after --mach / --alpha\n"
        "                                   (config key wall_temperature_ratio)\n"
        "  --wall-heat-flux=Q               With --no-slip: the wall feeds the heat flux Q into the fluid, of either sign (config key\n"
        "                                   wall_heat_flux).  The three exclude each other\n"
        "  --face-gradient=averaged|corrected  The face gradient of the viscous and Spalart-Allmaras diffusion: the average of the\n"
        "                                   two node gradients (the default), or that with its along-edge component replaced by the\n"
        "                                   two-point difference, which damps odd-even modes; corrected takes --viscous-cfl 0.2\n"
        "                                   unless said otherwise (config key face_gradient).  Needs the viscous terms.  One GPU\n"
        "  --loads-heat                     With --loads-friction: surface_loads.* and polar.csv rows gain Q (the heat rate the fluid\n"
        "                                   receives from the wall), A (the wall's area) and St_mean; surface.* rows gain qw, T and\n"
        "                                   St (config key loads_heat = Y).  One GPU\n"
        "  --polar=A0:A1:N                  N angles of attack from A0 to A1 inclusive, -g cycles each: the first starts from its\n"
        "                                   far field, every later one from the flow of the angle before it.  Writes polar.*\n"
        "                                   (CSV: alpha,mach,rms_last, the loads and coefficients of each angle's last cycle);\n"
        "                                   the dumps and surface_loads.* are the last angle's.  One GPU, or --gpus N with\n"
        "                                   --gpus-partition\n"
        "  --time-step=MODE                 reference (default: what the mesh name selects), global, local or local-legacy\n"
        "                                   (config key time_step); with --gpus N, --polar and --output-loads alike\n"
        "  --cfl=X                          CFL number of the time step, finite and above zero (default 0.5, the reference's;\n"
        "                                   config key cfl)\n"
        "  --residual-smoothing=EPS         implicit residual smoothing with coefficient EPS, finite and above zero (config key\n"
        "                                   residual_smoothing): every stage's update goes through Jacobi iterations over the edge\n"
        "                                   graph, which lets --cfl be two or more times as large.  One GPU, or --gpus N with one\n"
        "                                   multigrid level per GPU; not with --gpus-partition or a level split over GPUs\n"
        "  --smoothing-iterations=N         its Jacobi iterations, 0 ... 8 (default 2; 0 = off; config key smoothing_iterations)\n"
        "  --jst                            JST dissipation (config key jst = Y): the first-difference dissipation is kept only where a\n"
        "                                   pressure sensor sees a shock, a small fourth difference takes over elsewhere; with\n"
        "                                   kappa2 = 2.5, kappa4 = 0.15625 on level 0 unless said otherwise.  One GPU, or --gpus N with\n"
        "                                   one multigrid level per GPU; not with --gpus-partition or a level split over GPUs\n"
        "  --fas                            FAS multigrid (config key fas = Y): the coarse levels carry the fine level's residual as a\n"
        "                                   forcing term and return a correction, so the V-cycles converge to the fine grid's steady\n"
        "                                   state; one GPU, an input of two levels or more\n"
        "  --cycle=V|W|F                    The shape of the multigrid cycle (default V, the reference's): W visits every coarser level\n"
        "                                   twice per visit, F once as itself and once as a V-cycle; the coarsest level once per\n"
        "                                   down leg.  One GPU\n"
        "  --pre-sweeps=LIST                Sweeps per level before the restriction, 1 ... 8 (default 1): comma separated, one value\n"
        "                                   per level, or one value for all levels.  One GPU\n"
        "  --post-sweeps=LIST               Sweeps per level after the prolongation, 0 ... 8 (default 0 on level 0, 1 on the others):\n"
        "                                   one value per level, or one value for all levels but the coarsest, which has none.  One GPU\n"
        "  --fmg-cycles=LIST                A full-multigrid start before the -g cycles: the state is restricted to every level, then\n"
        "                                   from the coarsest level up LIST cycles run from that level and its state is interpolated\n"
        "                                   onto the next finer one.  One value per level 1 ... n-1, or one value for all, 0 ... 4096.\n"
        "                                   One GPU; not with --physical-time-step or --polar\n"
        "  --upwind                         upwind fluxes (config key upwind = Y): Roe's flux-difference splitting on the internal edges\n"
        "                                   in place of the reference's central flux and scalar dissipation, on limited MUSCL states;\n"
        "                                   one GPU; not on a level --jst covers\n"
        "  --upwind-levels=N                the multigrid levels 0 ... N-1 it runs on (default 1; 0 = off; config key upwind_levels)\n"
        "  --muscl-levels=N                 the levels 0 ... N-1 that reconstruct (default: every upwind level; they need .coords files;\n"
        "                                   the others are first order; config key muscl_levels)\n"
        "  --limiter=NAME                   none, barth-jespersen or venkatakrishnan (the default; config key limiter)\n"
        "  --venkat-k=X                     Venkatakrishnan's constant, above zero (default 5; config key venkat_k)\n"
        "  --entropy-fix=X                  Harten's fraction 0 ... 1, 0 = none (default 0.1; config key entropy_fix); each of the five\n"
        "                                   values implies --upwind\n"
        "  --jst-kappa2=X                   its second-difference coefficient, finite, zero or above, in units of the reference's\n"
        "                                   dissipation (config key jst_kappa2; implies --jst)\n"
        "  --jst-kappa4=X                   its fourth-difference coefficient, likewise (config key jst_kappa4; implies --jst)\n"
        "  --jst-levels=N                   the multigrid levels 0 ... N-1 it runs on (default 1; 0 = off; config key jst_levels;\n"
        "                                   implies --jst)\n"
        "  --viscosity=MU                   laminar viscous terms with dynamic viscosity MU, finite and above zero, in the solver's units\n"
        "                                   (config key viscosity): Navier-Stokes stresses and heat conduction added to every stage's\n"
        "                                   fluxes on level 0 unless said otherwise, and a viscous limit on the step.  One GPU, or --gpus N\n"
        "                                   with one multigrid level per GPU; not with --gpus-partition or a level split over GPUs\n"
        "  --reynolds=RE                    the same with MU = rho_inf * |V_inf| * L / RE of the free stream in use (after --mach / --alpha;\n"
        "                                   config key reynolds); not together with --viscosity\n"
        "  --ref-length=L                   the length L of --reynolds (default 1; config key ref_length)\n"
        "  --prandtl=X                      the Prandtl number (default 0.72; config key prandtl)\n"
        "  --no-slip                        solid walls are no-slip and adiabatic: momentum zero at their nodes (config key no_slip = Y;\n"
        "                                   default: slip walls, as without viscosity)\n"
        "  --viscous-cfl=X                  the step factors are limited to X * rho * h^2 / (max(4/3, gamma / Pr) * MU) (default 0.25;\n"
        "                                   config key viscous_cfl)\n"
        "  --viscous-levels=N               the multigrid levels 0 ... N-1 the viscous terms run on (default 1; 0 = off; config key\n"
        "                                   viscous_levels)\n"
        "  --sutherland                     with the viscous terms: Sutherland's law mu(T), T = p / rho (config key sutherland = Y); one GPU\n"
        "  --sutherland-tref=X              the T at which mu(T) = MU (default: the free stream's p / rho; config key sutherland_tref)\n"
        "  --sutherland-s=X                 Sutherland's constant over the reference temperature (default 0.3831; config key sutherland_s)\n"
        "  --smagorinsky[=CS]               with the viscous terms: the Smagorinsky eddy viscosity, constant CS (default 0.17), filter width\n"
        "                                   cbrt(volume), no wall damping (config key smagorinsky = Y or CS); one GPU\n"
        "  --prandtl-turbulent=X            the turbulent Prandtl number (default 0.9; config key prandtl_turbulent)\n"
        "  --spalart-allmaras[=RATIO]       with the viscous terms: the Spalart-Allmaras model (noft2), nu_tilde transported on level 0 and\n"
        "                                   restricted to the coarser viscous levels; RATIO = free-stream nu_tilde / nu, default 3 (config key\n"
        "                                   spalart_allmaras = Y or RATIO); needs .coords files; one GPU; not with --smagorinsky; with\n"
        "                                   --physical-time-step only together with --sa-time-accurate\n"
        "  --sa-time-accurate               with --spalart-allmaras: nu_tilde takes the BDF source of --physical-time-step (config key sa_time_accurate = Y)\n"
        "  --sa-length=wall|des|ddes        with --spalart-allmaras: the model length, the wall distance (default), DES97 or delayed DES (config key sa_length)\n"
        "  --sa-cdes=X                      ... and its constant, finite and above zero, default 0.65 (config key sa_cdes)\n"
        "  --wall-damping[=KAPPA]           with --smagorinsky: the length scale min(CS cbrt(volume), KAPPA d), d the distance to the nearest\n"
        "                                   solid-wall node, KAPPA default 0.41 (config key wall_damping = Y or KAPPA); needs .coords files\n"
        "  --physical-time-step=DT          dual time stepping: a time-accurate run with physical step DT, finite and above zero\n"
        "                                   (config key physical_time_step): BDF2 in physical time, every step solved in pseudo-time\n"
        "                                   by -g cycles (-g becomes the cycles PER PHYSICAL STEP; an RMS line per cycle as ever,\n"
        "                                   --output-loads one row per physical step, --output-variables the final state).  One GPU,\n"
        "                                   or --gpus N with one multigrid level per GPU; not with --gpus-partition, a level split\n"
        "                                   over GPUs or --polar\n"
        "  --time-steps=N                   its number of physical steps (default 1; config key time_steps)\n"
        "  --dual-time-clamp=X              the pseudo step is clamped to X * DT / volume (default 2/3; config key dual_time_clamp)\n"
        "  --bdf-order=1|2                  1 keeps the first-order formula throughout (default 2: BDF1 on the first step, then BDF2;\n"
        "                                   config key bdf_order)\n"
        "  --output-statistics              with --physical-time-step: time means and Reynolds stresses of level 0, one sample of\n"
        "                                   weight DT per physical step, into statistics.* (CSV): node, x, y, z, the means of\n"
        "                                   rho u v w p mut, Ruu Rvv Rww Ruv Ruw Rvw, p_rms, k.  With --output-surface also\n"
        "                                   surface_statistics.* (CSV): mean and rms of Cp and Cf per wall node.  One GPU\n"
        "  --statistics-start=K             the first K physical steps are not sampled (default 0; below --time-steps)\n");
}

bool parse_arguments(int argc, char **argv, Config &c)
{
    // src/Base/config.cpp:32-47,219-259.  (The reference stores the three --output-* flags
    // through bool-to-int* casts, so each one also clobbers the bools after it; here every
    // flag sets exactly its own field.)
    static const option long_opts[] = {
        {"help", no_argument, nullptr, 'h'},
        {"config-filepath", required_argument, nullptr, 'c'},
        {"input-file", required_argument, nullptr, 'i'},
        {"input-directory", required_argument, nullptr, 'd'},
        {"papi_config_file", required_argument, nullptr, 'p'},
        {"output-file-prefix", required_argument, nullptr, 'o'},
        {"mesh-duplicate-count", required_argument, nullptr, 'm'},
        {"num-cycles", required_argument, nullptr, 'g'},
        {"validate-result", no_argument, nullptr, 'v'},
        {"output-variables", no_argument, nullptr, 1001},
        {"output-fluxes", no_argument, nullptr, 1002},
        {"output-step-factors", no_argument, nullptr, 1003},
        {"device", required_argument, nullptr, 1004},
        {"no-timers", no_argument, nullptr, 1005},
        {"no-indirect-rw", no_argument, nullptr, 1006},
        {"fast", no_argument, nullptr, 1007},
        {"legacy-ordering", no_argument, nullptr, 1008},
        {"gpus", required_argument, nullptr, 1009},
        {"gpus-share-device", no_argument, nullptr, 1010},
        {"loop-timers", no_argument, nullptr, 1011},
        {"gpus-partition", no_argument, nullptr, 1012},
        {"output-loads", no_argument, nullptr, 1013},
        {"loads-reference", required_argument, nullptr, 1014},
        {"mach", required_argument, nullptr, 1015},
        {"alpha", required_argument, nullptr, 1016},
        {"polar", required_argument, nullptr, 1017},
        {"time-step", required_argument, nullptr, 1018},
        {"cfl", required_argument, nullptr, 1019},
        {"residual-smoothing", required_argument, nullptr, 1020},
        {"smoothing-iterations", required_argument, nullptr, 1021},
        {"physical-time-step", required_argument, nullptr, 1022},
        {"time-steps", required_argument, nullptr, 1023},
        {"dual-time-clamp", required_argument, nullptr, 1024},
        {"bdf-order", required_argument, nullptr, 1025},
        {"jst", no_argument, nullptr, 1026},
        {"fas", no_argument, nullptr, 1030},
        {"cycle", required_argument, nullptr, 1050},
        {"pre-sweeps", required_argument, nullptr, 1051},
        {"post-sweeps", required_argument, nullptr, 1052},
        {"fmg-cycles", required_argument, nullptr, 1053},
        {"jst-kappa2", required_argument, nullptr, 1027},
        {"jst-kappa4", required_argument, nullptr, 1028},
        {"jst-levels", required_argument, nullptr, 1029},
        {"viscosity", required_argument, nullptr, 1031},
        {"reynolds", required_argument, nullptr, 1032},
        {"ref-length", required_argument, nullptr, 1033},
        {"prandtl", required_argument, nullptr, 1034},
        {"viscous-cfl", required_argument, nullptr, 1035},
        {"no-slip", no_argument, nullptr, 1036},
        {"viscous-levels", required_argument, nullptr, 1037},
        {"sutherland", no_argument, nullptr, 1040},
        {"sutherland-tref", required_argument, nullptr, 1041},
        {"sutherland-s", required_argument, nullptr, 1042},
        {"prandtl-turbulent", required_argument, nullptr, 1043},
        {"smagorinsky", optional_argument, nullptr, 1044},
        {"wall-damping", optional_argument, nullptr, 1045},
        {"spalart-allmaras", optional_argument, nullptr, 1046},
        {"loads-friction", no_argument, nullptr, 1038},
        {"output-surface", no_argument, nullptr, 1039},
        {"wall-temperature", required_argument, nullptr, 1047},
        {"wall-temperature-ratio", required_argument, nullptr, 1048},
        {"wall-heat-flux", required_argument, nullptr, 1049},
        {"loads-heat", no_argument, nullptr, 1054},
        {"face-gradient", required_argument, nullptr, 1055},
        {"sa-time-accurate", no_argument, nullptr, 1056},
        {"sa-length", required_argument, nullptr, 1057},
        {"sa-cdes", required_argument, nullptr, 1058},
        {"output-statistics", no_argument, nullptr, 1059},
        {"statistics-start", required_argument, nullptr, 1060},
        {"upwind", no_argument, nullptr, 1061},
        {"upwind-levels", required_argument, nullptr, 1062},
        {"muscl-levels", required_argument, nullptr, 1063},
        {"limiter", required_argument, nullptr, 1064},
        {"venkat-k", required_argument, nullptr, 1065},
        {"entropy-fix", required_argument, nullptr, 1066},
        {nullptr, 0, nullptr, 0}};
    int optc;
    while ((optc = getopt_long(argc, argv, "hc:i:d:p:o:m:g:v", long_opts, nullptr)) != -1) {
        switch (optc) {
            case 'h': print_help(); return false;
            case 'i': c.input_file = optarg; break;
            case 'c': c.config_filepath = optarg; read_config(c); break;
            case 'd': c.input_file_directory = optarg; break;
            case 'p': c.papi_config_file = optarg; break;
            case 'o': c.output_file_prefix = optarg; break;
            case 'm': c.mesh_duplicate_count = std::atoi(optarg); break;
            case 'g': c.num_cycles = std::atoi(optarg); break;
            case 'v': c.validate_result = true; break;
            case 1001: c.output_variables = true; break;
            case 1002: c.output_fluxes = true; break;
            case 1003: c.output_step_factors = true; break;
            case 1004: c.device = std::atoi(optarg); break;
            case 1005: c.timers = false; break;
            case 1006: c.indirect_rw = false; break;
            case 1007: c.fast_math = true; break;
            case 1008: c.legacy_ordering = true; break;
            case 1009: c.gpus = std::atoi(optarg); break;
            case 1010: c.gpus_share_device = true; break;
            case 1011: c.loop_timers = true; break;
            case 1012: c.gpus_partition = true; break;
            case 1013: c.output_loads = true; break;
            case 1014:
                if (!parse_loads_reference(optarg, c.loads_ref)) {
                    std::fprintf(stderr, "ERROR: --loads-reference=%s: expected S,c,x,y,z (five numbers, S and c positive)\n", optarg);
                    return false;
                }
                break;
            case 1015:
            case 1016:
                if (!parse_number(optarg, optc == 1015 ? &c.ff_mach : &c.angle_of_attack)) {
                    std::fprintf(stderr, "ERROR: --%s=%s: expected a number\n", optc == 1015 ? "mach" : "alpha", optarg);
                    return false;
                }
                c.free_stream_given = true;
                break;
            case 1017:
                if (!parse_polar(optarg, c)) {
                    std::fprintf(stderr, "ERROR: --polar=%s: expected A0:A1:N (two angles in degrees and a count of at least 1)\n", optarg);
                    return false;
                }
                break;
            case 1018:
                if (!parse_time_step_mode(optarg, &c.time_step_mode)) {
                    std::fprintf(stderr, "ERROR: --time-step=%s: expected reference, global, local or local-legacy\n", optarg);
                    return false;
                }
                c.time_step_given = true;
                break;
            case 1019:
                if (!parse_positive(optarg, &c.cfl)) {
                    std::fprintf(stderr, "ERROR: --cfl=%s: expected a finite number above zero\n", optarg);
                    return false;
                }
                c.time_step_given = true;
                break;
            case 1020:
                if (!parse_positive(optarg, &c.smoothing_eps)) {
                    std::fprintf(stderr, "ERROR: --residual-smoothing=%s: expected a finite number above zero\n", optarg);
                    return false;
                }
                c.smoothing_given = true;
                break;
            case 1021:
                if (!parse_smoothing_iterations(optarg, &c.smoothing_iterations)) {
                    std::fprintf(stderr, "ERROR: --smoothing-iterations=%s: expected a whole number 0 ... %d\n", optarg, MGCFD_MAX_SMOOTHING_ITERATIONS);
                    return false;
                }
                c.smoothing_iterations_given = true;
                break;
            case 1022:
                if (!parse_positive(optarg, &c.dual_dt)) {
                    std::fprintf(stderr, "ERROR: --physical-time-step=%s: expected a finite number above zero\n", optarg);
                    return false;
                }
                c.dual_given = true;
                break;
            case 1023:
                if (!parse_whole(optarg, 1, kMaxTimeSteps, &c.time_steps)) {
                    std::fprintf(stderr, "ERROR: --time-steps=%s: expected a whole number 1 ... %d\n", optarg, kMaxTimeSteps);
                    return false;
                }
                c.dual_extras_given = true;
                break;
            case 1024:
                if (!parse_positive(optarg, &c.dual_clamp)) {
                    std::fprintf(stderr, "ERROR: --dual-time-clamp=%s: expected a finite number above zero\n", optarg);
                    return false;
                }
                c.dual_extras_given = true;
                break;
            case 1025:
                if (!parse_whole(optarg, 1, 2, &c.bdf_order)) {
                    std::fprintf(stderr, "ERROR: --bdf-order=%s: expected 1 or 2\n", optarg);
                    return false;
                }
                c.dual_extras_given = true;
                break;
            case 1026: c.jst_given = true; break;
            case 1030: c.fas = true; break;
            case 1061: c.upwind_given = true; break;
            case 1062:
            case 1063:
                if (!parse_whole(optarg, 0, kMaxJstLevels, optc == 1062 ? &c.upwind_levels : &c.muscl_levels_said)) {
                    std::fprintf(stderr, "ERROR: --%s-levels=%s: expected a whole number 0 ... %d\n", optc == 1062 ? "upwind" : "muscl", optarg, kMaxJstLevels);
                    return false;
                }
                c.upwind_given = true;
                break;
            case 1064:
                if (!set_limiter(c, optarg)) {
                    std::fprintf(stderr, "ERROR: --limiter=%s: expected none, barth-jespersen or venkatakrishnan\n", optarg);
                    return false;
                }
                break;
            case 1065:
                if (!parse_positive(optarg, &c.venkat_k)) {
                    std::fprintf(stderr, "ERROR: --venkat-k=%s: expected a finite number above zero\n", optarg);
                    return false;
                }
                c.upwind_given = true;
                break;
            case 1066:
                if (!parse_not_negative(optarg, &c.entropy_fix) || c.entropy_fix > 1.0) {
                    std::fprintf(stderr, "ERROR: --entropy-fix=%s: expected a number 0 ... 1\n", optarg);
                    return false;
                }
                c.upwind_given = true;
                break;
            case 1050: {
                const std::string v(optarg);
                if (v == "V" || v == "v") c.cycle_shape = MGCFD_CYCLE_V;
                else if (v == "W" || v == "w") c.cycle_shape = MGCFD_CYCLE_W;
                else if (v == "F" || v == "f") c.cycle_shape = MGCFD_CYCLE_F;
                else { std::fprintf(stderr, "ERROR: --cycle=%s: expected V, W or F\n", optarg); return false; }
                break;
            }
            case 1051:
                if (!parse_whole_list(optarg, 1, MGCFD_MAX_CYCLE_SWEEPS, &c.pre_sweeps)) {
                    std::fprintf(stderr, "ERROR: --pre-sweeps=%s: expected whole numbers 1 ... %d, comma separated\n", optarg, MGCFD_MAX_CYCLE_SWEEPS);
                    return false;
                }
                break;
            case 1052:
                if (!parse_whole_list(optarg, 0, MGCFD_MAX_CYCLE_SWEEPS, &c.post_sweeps)) {
                    std::fprintf(stderr, "ERROR: --post-sweeps=%s: expected whole numbers 0 ... %d, comma separated\n", optarg, MGCFD_MAX_CYCLE_SWEEPS);
                    return false;
                }
                break;
            case 1053:
                if (!parse_whole_list(optarg, 0, MGCFD_MAX_ADVANCE_CYCLES, &c.fmg_cycles)) {
                    std::fprintf(stderr, "ERROR: --fmg-cycles=%s: expected whole numbers 0 ... %d, comma separated\n", optarg, MGCFD_MAX_ADVANCE_CYCLES);
                    return false;
                }
                break;
            case 1027:
            case 1028:
                if (!parse_not_negative(optarg, optc == 1027 ? &c.jst_kappa2 : &c.jst_kappa4)) {
                    std::fprintf(stderr, "ERROR: --jst-kappa%d=%s: expected a finite number, zero or above\n", optc == 1027 ? 2 : 4, optarg);
                    return false;
                }
                c.jst_given = true;
                break;
            case 1029:
                if (!parse_whole(optarg, 0, kMaxJstLevels, &c.jst_levels)) {
                    std::fprintf(stderr, "ERROR: --jst-levels=%s: expected a whole number 0 ... %d\n", optarg, kMaxJstLevels);
                    return false;
                }
                c.jst_given = true;
                break;
            case 1031: case 1032: case 1033: case 1034: case 1035: {
                static const char *const names[] = {"viscosity", "reynolds", "ref-length", "prandtl", "viscous-cfl"};
                double *const dst[] = {&c.viscosity, &c.reynolds, &c.ref_length, &c.prandtl, &c.viscous_cfl};
                if (!parse_positive(optarg, dst[optc - 1031])) {
                    std::fprintf(stderr, "ERROR: --%s=%s: expected a finite number above zero\n", names[optc - 1031], optarg);
                    return false;
                }
                if (optc == 1031) c.viscosity_given = true; else if (optc == 1032) c.reynolds_given = true; else c.viscous_extras_given = true;
                if (optc == 1035) c.viscous_cfl_given = true;
                break;
            }
            case 1036: c.no_slip = true; c.viscous_extras_given = true; break;
            case 1037:
                if (!parse_whole(optarg, 0, kMaxJstLevels, &c.viscous_levels)) {
                    std::fprintf(stderr, "ERROR: --viscous-levels=%s: expected a whole number 0 ... %d\n", optarg, kMaxJstLevels);
                    return false;
                }
                c.viscous_extras_given = true;
                break;
            case 1038: c.loads_friction = true; break;
            case 1040: c.sutherland = true; break;
            case 1041: case 1042: case 1043: {
                static const char *const names[] = {"sutherland-tref", "sutherland-s", "prandtl-turbulent"};
                double *const dst[] = {&c.sutherland_tref, &c.sutherland_s, &c.prandtl_turbulent};
                if (!parse_positive(optarg, dst[optc - 1041])) {
                    std::fprintf(stderr, "ERROR: --%s=%s: expected a finite number above zero\n", names[optc - 1041], optarg);
                    return false;
                }
                c.model_extras_given = true;
                break;
            }
            case 1044: {
                // --smagorinsky, --smagorinsky=CS or --smagorinsky CS (the next word, where it does not start another option)
                const char *arg = optarg;
                if (!arg && optind < argc && argv[optind][0] != '-') arg = argv[optind++];
                if (arg && !parse_positive(arg, &c.smagorinsky_cs)) {
                    std::fprintf(stderr, "ERROR: --smagorinsky=%s: expected a finite constant above zero\n", arg);
                    return false;
                }
                c.smagorinsky = true;
                break;
            }
            case 1045: {
                // --wall-damping, --wall-damping=KAPPA or --wall-damping KAPPA, as --smagorinsky takes its constant
                const char *arg = optarg;
                if (!arg && optind < argc && argv[optind][0] != '-') arg = argv[optind++];
                if (arg && !parse_positive(arg, &c.wall_kappa)) {
                    std::fprintf(stderr, "ERROR: --wall-damping=%s: expected a finite constant above zero\n", arg);
                    return false;
                }
                c.wall_damping = true;
                break;
            }
            case 1046: {
                // --spalart-allmaras, --spalart-allmaras=RATIO or --spalart-allmaras RATIO, as --smagorinsky takes its constant
                const char *arg = optarg;
                if (!arg && optind < argc && argv[optind][0] != '-') arg = argv[optind++];
                if (arg && !parse_positive(arg, &c.sa_ratio)) {
                    std::fprintf(stderr, "ERROR: --spalart-allmaras=%s: expected a finite ratio above zero\n", arg);
                    return false;
                }
                c.spalart_allmaras = true;
                break;
            }
            case 1039: c.output_surface = true; break;
            case 1047: case 1048: case 1049: {
                static const char *const names[] = {"wall-temperature", "wall-temperature-ratio", "wall-heat-flux"};
                if (!set_wall_thermal(c, optc - 1047, optarg)) {
                    std::fprintf(stderr, "ERROR: --%s=%s: expected a finite number%s\n", names[optc - 1047], optarg, optc == 1049 ? "" : " above zero");
                    return false;
                }
                break;
            }
            case 1054: c.loads_heat = true; break;
            case 1055:
                if (!set_face_gradient(c, optarg)) {
                    std::fprintf(stderr, "ERROR: --face-gradient=%s: expected averaged or corrected\n", optarg);
                    return false;
                }
                break;
            case 1056: c.sa_time_accurate = true; c.sa_unsteady_given = true; break;
            case 1057:
                if (!set_sa_length(c, optarg)) {
                    std::fprintf(stderr, "ERROR: --sa-length=%s: expected wall, des or ddes\n", optarg);
                    return false;
                }
                c.sa_unsteady_given = true;
                break;
            case 1058:
                if (!parse_positive(optarg, &c.sa_cdes)) {
                    std::fprintf(stderr, "ERROR: --sa-cdes=%s: expected a finite number above zero\n", optarg);
                    return false;
                }
                c.sa_unsteady_given = true;
                break;
            case 1059: c.output_statistics = true; break;
            case 1060:
                if (!parse_whole(optarg, 0, kMaxTimeSteps, &c.statistics_start)) {
                    std::fprintf(stderr, "ERROR: --statistics-start=%s: expected a whole number 0 ... %d\n", optarg, kMaxTimeSteps);
                    return false;
                }
                c.statistics_start_given = true;
                break;
            default: std::printf("Unknown command line parameter '%c'\n", optc);
        }
    }
    if (c.smoothing_iterations_given && !c.smoothing_given && c.smoothing_iterations > 0) {
        std::fprintf(stderr, "ERROR: --smoothing-iterations needs --residual-smoothing EPS (the residual smoothing's coefficient)\n");
        return false;
    }
    if (c.viscosity_given && c.reynolds_given) {
        std::fprintf(stderr, "ERROR: --viscosity and --reynolds both set the viscosity: give one of them\n");
        return false;
    }
    if (c.viscous_extras_given && !c.viscous()) {
        std::fprintf(stderr, "ERROR: --ref-length, --prandtl, --no-slip, --viscous-cfl and --viscous-levels need --viscosity MU or --reynolds RE (the viscous terms)\n");
        return false;
    }
    if ((c.viscosity_model() || c.model_extras_given) && !c.viscous()) {
        std::fprintf(stderr, "ERROR: --sutherland, --smagorinsky and their companions need --viscosity MU or --reynolds RE (the viscous terms)\n");
        return false;
    }
    if (c.viscosity_model() && c.gpus > 1) {
        std::fprintf(stderr, "ERROR: the viscosity model (--sutherland, --smagorinsky) runs on one GPU only: not with --gpus N or --gpus-partition\n");
        return false;
    }
    if (c.spalart_allmaras && c.smagorinsky) {
        std::fprintf(stderr, "ERROR: --spalart-allmaras and --smagorinsky are two eddy-viscosity models: give one of them\n");
        return false;
    }
    if (c.sa_unsteady_given && !c.spalart_allmaras) {
        std::fprintf(stderr, "ERROR: --sa-time-accurate, --sa-length and --sa-cdes need --spalart-allmaras (they are settings of that model)\n");
        return false;
    }
    if (c.spalart_allmaras && c.dual_given && !c.sa_time_accurate) {
        std::fprintf(stderr, "ERROR: --spalart-allmaras does not run with --physical-time-step (nu_tilde has no physical-time source) unless --sa-time-accurate gives it one\n");
        return false;
    }
    if (c.wall_damping && !c.smagorinsky) {
        std::fprintf(stderr, "ERROR: --wall-damping needs --smagorinsky (it limits that model's length scale)\n");
        return false;
    }
    if (c.loads_friction && !(c.viscous() && c.viscous_levels > 0 && (c.output_loads || c.polar))) {
        std::fprintf(stderr, "ERROR: --loads-friction needs the viscous terms (--viscosity MU or --reynolds RE) and --output-loads or --polar\n");
        return false;
    }
    if ((c.loads_friction || c.output_surface) && c.gpus > 1) {
        std::fprintf(stderr, "ERROR: --loads-friction and --output-surface run on one GPU only\n");
        return false;
    }
    if (c.wall_thermal_flags > 1) {
        std::fprintf(stderr, "ERROR: --wall-temperature, --wall-temperature-ratio and --wall-heat-flux are three conditions of the one wall: give one of them\n");
        return false;
    }
    if (c.wall_thermal_flags > 0 && !(c.viscous() && c.viscous_levels > 0 && c.no_slip)) {
        std::fprintf(stderr, "ERROR: --wall-temperature, --wall-temperature-ratio and --wall-heat-flux need --no-slip and the viscous terms (--viscosity MU or --reynolds RE)\n");
        return false;
    }
    if (c.loads_heat && !c.loads_friction) {
        std::fprintf(stderr, "ERROR: --loads-heat needs --loads-friction (the heat loads stand behind the friction loads)\n");
        return false;
    }
    if ((c.wall_thermal_flags > 0 || c.loads_heat) && c.gpus > 1) {
        std::fprintf(stderr, "ERROR: the wall thermal conditions and --loads-heat run on one GPU only: not with --gpus N\n");
        return false;
    }
    if (c.upwind_given && c.muscl_levels() > c.upwind_levels) {
        std::fprintf(stderr, "ERROR: --muscl-levels %d exceeds --upwind-levels %d: a level reconstructs for the upwind flux only\n", c.muscl_levels(), c.upwind_levels);
        return false;
    }
    if (c.upwind_given && c.upwind_levels > 0 && c.jst_given && c.jst_levels > 0) {
        std::fprintf(stderr, "ERROR: --upwind and --jst on the same level: Roe's flux carries its own dissipation (give one of them, or --jst-levels 0)\n");
        return false;
    }
    if (c.upwind_given && c.upwind_levels > 0 && c.gpus > 1) {
        std::fprintf(stderr, "ERROR: the upwind flux (--upwind) runs on one GPU only: not with --gpus N or --gpus-partition (a level split over GPUs would need its limited gradient exchanged per stage)\n");
        return false;
    }
    if (c.face_gradient_given && !(c.viscous() && c.viscous_levels > 0)) {
        std::fprintf(stderr, "ERROR: --face-gradient needs the viscous terms (--viscosity MU or --reynolds RE): it is their face gradient\n");
        return false;
    }
    if (c.face_gradient_given && c.gpus > 1) {
        std::fprintf(stderr, "ERROR: --face-gradient runs on one GPU only: not with --gpus N\n");
        return false;
    }
    if (c.face_gradient == MGCFD_FACE_GRADIENT_CORRECTED && !c.viscous_cfl_given) c.viscous_cfl = MGCFD_VISCOUS_CFL_CORRECTED;   // (the corrected operator is stiffer)
    if (c.dual_extras_given && !c.dual_given) {
        std::fprintf(stderr, "ERROR: --time-steps, --dual-time-clamp and --bdf-order need --physical-time-step DT (dual time stepping)\n");
        return false;
    }
    if (c.statistics_start_given && !c.output_statistics) {
        std::fprintf(stderr, "ERROR: --statistics-start needs --output-statistics (it is the step the statistics begin behind)\n");
        return false;
    }
    if (c.output_statistics && !c.dual_given) {
        std::fprintf(stderr, "ERROR: --output-statistics needs --physical-time-step DT (the statistics are time averages of a dual-time run)\n");
        return false;
    }
    if (c.output_statistics && c.gpus > 1) {
        std::fprintf(stderr, "ERROR: --output-statistics runs on one GPU only: not with --gpus N\n");
        return false;
    }
    if (c.output_statistics && c.statistics_start >= c.time_steps) {
        std::fprintf(stderr, "ERROR: --statistics-start=%d: must be below --time-steps (%d), or no step is sampled\n", c.statistics_start, c.time_steps);
        return false;
    }
    if (c.dual_given && (c.num_cycles < 1 || c.num_cycles > MGCFD_MAX_ADVANCE_CYCLES)) {
        std::fprintf(stderr, "ERROR: dual time stepping (--physical-time-step): -g is the cycles per physical step, 1 ... %d\n", MGCFD_MAX_ADVANCE_CYCLES);
        return false;
    }
    return !c.config_bad;
}

// src/Base/io_enhanced.cpp:26-74
std::string filename_suffix(const Config &c, int level)
{
    std::string s = "size=" + std::to_string(c.mesh_duplicate_count) + "x.cycles=" + std::to_string(c.num_cycles);
    if (level >= 0) s += ".level=" + std::to_string(level);
    return s;
}
std::string output_filepath(const Config &c, const std::string &name, int level)
{
    std::string p = c.output_file_prefix;
    if (!p.empty() && p.back() != '/') p += ".";
    return p + name + "." + filename_suffix(c, level);
}
std::string solution_filepath(const Config &c, const std::string &name, int level)
{
    std::string p = c.input_file_directory;
    if (!p.empty() && p.back() != '/') p += "/";
    return p + "solution." + name + "." + filename_suffix(c, level);
}
std::string csv_filepath(const Config &c, const char *name)
{
    std::string p = c.output_file_prefix;
    if (!p.empty() && p.back() != '/') p += ".";
    return p + name;
}

const char *mesh_name(int v)
{
    switch (v) {
        case MGCFD_MESH_LA_CASCADE: return "la_cascade";
        case MGCFD_MESH_ROTOR_37: return "rotor37";
        case MGCFD_MESH_FVCORR: return "fvcorr";
        case MGCFD_MESH_M6_WING: return "m6wing";
        default: return "unknown";
    }
}

#define STR2(x) #x
#define STR(x) STR2(x)

// The 16 identification columns of src/Base/io_enhanced.cpp:858-1016, re-read for a GPU build:
// CC = hipcc's clang, Instruction set = gfx950, Num threads = number of GPUs, CPU = device name.
void csv_identification(const Config &c, int size, int mesh_variant, const std::string &device_name,
                        std::string &header, std::string &line, int num_gpus = 1)
{
    std::ostringstream h, d;
    h << "Size,";                  d << size << ",";
    h << "Mesh,";                  d << mesh_name(mesh_variant) << ",";
    h << "MG cycles,";             d << c.num_cycles << ",";
    h << "Flux variant,";          d << "Normal,";
    // (the reference leaves the column empty for a plain build; here it says how the per-loop times were obtained)
    h << "Flux options,";          d << (c.timers && !c.loop_timers && num_gpus == 1 ? "fused stages; loop times attributed from every 32nd sweep run per loop" : "") << ",";
    h << "CC,";                    d << "hipcc,";
    h << "CC version,";            d << STR(__clang_major__) "." STR(__clang_minor__) "." STR(__clang_patchlevel__) ",";
    h << "Opt level,";             d << "3,";
    h << "Instruction set,";       d << "gfx950,";
    h << "SIMD,";                  d << "N,";
    h << "SIMD len,";              d << "1,";
    h << "OpenMP,";                d << "Off,";
    h << "Num threads,";           d << num_gpus << ",";
    h << "Permit scatter OpenMP,"; d << "N,";
    h << "Flux fission,";          d << "N,";
    h << "CPU,";                   d << device_name << ",";
    header = h.str();
    line = d.str();
}

void write_csv(const std::string &path, const std::string &ident_header, const std::string &ident_line, int levels,
               const std::vector<std::vector<std::string>> &cells, bool with_total, double total)
{
    std::remove(path.c_str());
    std::ofstream out(path);
    static const char *cols[MGCFD_NUM_LOOPS] = {"flux", "update", "compute_step", "time_step", "restrict", "prolong", "indirect_rw"};
    out << ident_header << "ThreadNum,CpuId,";
    for (int l = 0; l < levels; l++)
        for (int k = 0; k < MGCFD_NUM_LOOPS; k++) out << cols[k] << l << ",";
    if (with_total) out << "Total,";
    out << std::endl;
    out << ident_line << 0 << "," << sched_getcpu() << ",";
    for (int l = 0; l < levels; l++)
        for (int k = 0; k < MGCFD_NUM_LOOPS; k++) out << cells[l][k] << ",";
    if (with_total) out << total << ",";
    out << std::endl;
}

int fail(const char *what)
{
    std::fprintf(stderr, "ERROR: %s: %s\n", what, mgcfd_last_error());
    return EXIT_FAILURE;
}

// What the reference does between its cycle loop and its CSV files (src/euler3d_cpu_double.cpp:704-772), for one GPU or
// several: -v / validate_result = Y (NaN check of every level, then level 0 against the solution file with
// identify_differences' tolerance) and the level-0 dumps.  get(which, ncols, out) reads a level-0 array of the WHOLE mesh in
// original numbering; nan_check(level, &cell) is check_for_invalid_variables on that level.  Returns 0 or EXIT_FAILURE.
template <typename Get, typename NanCheck>
int validate_and_dump(const Config &conf, int levels, int mesh_variant, int64_t nel0, Get &&get, NanCheck &&nan_check)
{
    std::printf("\n");
    if (conf.validate_result) {
        std::printf("Beginning validation of variables[]\n");
        for (int l = 0; l < levels; l++) {
            int64_t bad = -1;
            if (nan_check(l, &bad) != MGCFD_OK) {
                std::printf("\nERROR: NaN detected!\nCell %ld\n", (long)bad);
                return EXIT_FAILURE;
            }
        }
        std::printf("  NaN check passed\n");
        bool passed = true;
        const std::string sol = solution_filepath(conf, "variables", 0);
        std::ifstream file(sol);
        if (!file.is_open()) {
            std::printf("  could not open variables solution file:\n    %s\n  aborting validation\n", sol.c_str());
            passed = false;
        } else {
            std::vector<double> variables(static_cast<size_t>(nel0) * MGCFD_NVAR), master(variables.size());
            for (auto &v : master) file >> v;
            if (get(MGCFD_ARR_VARIABLES, MGCFD_NVAR, variables.data()) != MGCFD_OK) return fail("reading back variables");
            std::printf("  scanning variables[] on level 0 for errors\n");
            int64_t first_bad = -1;
            if (mgcfd_identify_differences(variables.data(), master.data(), nel0, mesh_variant, &first_bad) != MGCFD_OK) {
                std::printf("ERROR: Unacceptable error detected at (i=%ld, v=%d)\n", (long)(first_bad / MGCFD_NVAR), int(first_bad % MGCFD_NVAR));
                std::printf("       - incorrect value = %.23f\n", variables[static_cast<size_t>(first_bad)]);
                std::printf("       - correct value =   %.23f\n", master[static_cast<size_t>(first_bad)]);
                return EXIT_FAILURE;
            }
        }
        if (passed) std::printf("PASS: variables[] validated successfully\n");
        std::printf("\n");
    }
    // ---- dumps, level 0 only (src/euler3d_cpu_double.cpp:752-772) ----
    auto dump = [&](int which, const char *name, int ncols) -> int {
        std::vector<double> a(static_cast<size_t>(nel0) * ncols);
        if (get(which, ncols, a.data()) != MGCFD_OK) return fail("reading back an array");
        const std::string path = output_filepath(conf, name, 0);
        if (which == MGCFD_ARR_VARIABLES) std::printf("Dumping variables[] to file: %s\n", path.c_str());
        if (mgcfd_write_array(path.c_str(), a.data(), nel0, ncols) != MGCFD_OK) return fail("writing a dump");
        return 0;
    };
    if (conf.output_variables && dump(MGCFD_ARR_VARIABLES, "variables", MGCFD_NVAR)) return EXIT_FAILURE;
    if (conf.output_step_factors && dump(MGCFD_ARR_STEP_FACTORS, "step_factors", 1)) return EXIT_FAILURE;
    if (conf.output_fluxes && dump(MGCFD_ARR_FLUXES, "fluxes", MGCFD_NVAR)) return EXIT_FAILURE;
    if (conf.output_volumes && dump(MGCFD_ARR_VOLUMES, "volumes", 1)) return EXIT_FAILURE;
    return 0;
}

// The loads columns of a surface_loads.* or polar.csv row: Fx ... Mz and CD ... CMz; with --loads-friction `row` holds the
// pressure six and the friction six, the twelve columns are those of their total (one addition per component) and the friction
// loads and their coefficients follow.
const char *const kFrictionColumns = ",Fxv,Fyv,Fzv,Mxv,Myv,Mzv,CDv,CLv,CSv,CMxv,CMyv,CMzv";
// ... and with --loads-heat the heat rate the fluid receives from the wall, the wall's area and the mean Stanton number
// St_mean = (Q / A) / (rho_inf |V_inf| cp (T_total - Tw)), cp = GAMMA / (GAMMA - 1), Tw = the wall temperature of
// --wall-temperature[-ratio], the static free-stream temperature under any other wall
const char *const kHeatColumns = ",Q,A,St_mean";
std::string loads_header(const Config &conf) { return std::string(conf.loads_friction ? kFrictionColumns : "") + (conf.loads_heat ? kHeatColumns : ""); }
// the wall temperature of the run against the far field ff17: as given, or the ratio times the static free-stream temperature;
// *isothermal: the wall is held at it
int wall_temperature_of(const Config &conf, const double ff17[17], double *tw, bool *isothermal, double *t_total)
{
    double t_static = 0.0;
    const int rc = mgcfd_free_stream_temperature(ff17, &t_static, t_total);
    if (rc != MGCFD_OK) return rc;
    *isothermal = conf.wall_thermal_flags > 0 && conf.wall_mode == MGCFD_WALL_ISOTHERMAL;
    *tw = *isothermal ? (conf.wall_ratio ? conf.wall_value * t_static : conf.wall_value) : t_static;
    return MGCFD_OK;
}
// rho_inf |V_inf| cp
double stanton_scale(const double ff17[17])
{
    const double vx = ff17[1] / ff17[0], vy = ff17[2] / ff17[0], vz = ff17[3] / ff17[0];
    return ff17[0] * std::sqrt(vx * vx + vy * vy + vz * vz) * (1.4 / (1.4 - 1.0));
}
int write_loads_columns(FILE *f, const Config &conf, const double ff17[17], const double *row)
{
    double total[6], coef[6];
    for (int k = 0; k < 6; k++) total[k] = conf.loads_friction ? row[k] + row[6 + k] : row[k];
    if (mgcfd_load_coefficients(ff17, total, conf.loads_ref[0], conf.loads_ref[1], coef) != MGCFD_OK) return 1;
    for (int k = 0; k < 6; k++) std::fprintf(f, ",%.17e", total[k]);
    for (int k = 0; k < 6; k++) std::fprintf(f, ",%.17e", coef[k]);
    if (!conf.loads_friction) return 0;
    if (mgcfd_load_coefficients(ff17, row + 6, conf.loads_ref[0], conf.loads_ref[1], coef) != MGCFD_OK) return 1;
    for (int k = 0; k < 6; k++) std::fprintf(f, ",%.17e", row[6 + k]);
    for (int k = 0; k < 6; k++) std::fprintf(f, ",%.17e", coef[k]);
    if (!conf.loads_heat) return 0;
    double tw = 0.0, t_total = 0.0;
    bool isothermal = false;
    if (wall_temperature_of(conf, ff17, &tw, &isothermal, &t_total) != MGCFD_OK) return 1;
    std::fprintf(f, ",%.17e,%.17e,%.17e", row[12], row[13], (row[12] / row[13]) / (stanton_scale(ff17) * (t_total - tw)));
    return 0;
}

// --output-loads: one row per cycle (dual time stepping: per physical step), the loads and their coefficients (nothing on stdout: it stays the reference's)
int write_loads_csv(const Config &conf, const double ff17[17], const std::vector<double> &loads)
{
    const std::string path = output_filepath(conf, "surface_loads", 0);
    FILE *f = std::fopen(path.c_str(), "w");
    if (!f) return fail(("opening " + path).c_str());
    std::fprintf(f, "cycle,Fx,Fy,Fz,Mx,My,Mz,CD,CL,CS,CMx,CMy,CMz%s\n", loads_header(conf).c_str());
    for (int c = 0; c < conf.loads_rows(); c++) {
        std::fprintf(f, "%d", c + 1);
        if (write_loads_columns(f, conf, ff17, loads.data() + static_cast<size_t>(c) * conf.loads_width())) {
            std::fclose(f);
            return fail("computing the load coefficients");
        }
        std::fprintf(f, "\n");
    }
    if (std::fclose(f) != 0) return fail(("writing " + path).c_str());
    return 0;
}

// --polar: one row per angle — the RMS, loads and coefficients of its last cycle (nothing on stdout)
struct PolarRow { double alpha, mach, rms_last, loads[14], ff17[17]; };
int write_polar_csv(const Config &conf, const std::vector<PolarRow> &rows)
{
    const std::string path = csv_filepath(conf, "polar.csv");
    FILE *f = std::fopen(path.c_str(), "w");
    if (!f) return fail(("opening " + path).c_str());
    std::fprintf(f, "alpha,mach,rms_last,Fx,Fy,Fz,Mx,My,Mz,CD,CL,CS,CMx,CMy,CMz%s\n", loads_header(conf).c_str());
    for (const PolarRow &r : rows) {
        std::fprintf(f, "%.17e,%.17e,%.17e", r.alpha, r.mach, r.rms_last);
        if (write_loads_columns(f, conf, r.ff17, r.loads)) {
            std::fclose(f);
            return fail("computing the load coefficients");
        }
        std::fprintf(f, "\n");
    }
    if (std::fclose(f) != 0) return fail(("writing " + path).c_str());
    return 0;
}

// --output-surface: one row per wall node of level 0 in the state the run ends with — the node's original id and coordinates,
// the sum a of its solid-wall edge weights, Cp = dp / q_inf and the tangential friction coefficient
// Cf = (t - (t.n) n) / (|a| q_inf), n = a / |a| (mgcfd_wall_distribution; nothing on stdout)
int write_surface_csv(const Config &conf, mgcfd_solver *solver, const mgcfd_mesh *mesh)
{
    int64_t n = 0;
    double ff17[17];
    mgcfd_level_desc desc;
    if (mgcfd_wall_node_count(solver, 0, &n) != MGCFD_OK || mgcfd_get_far_field(solver, ff17) != MGCFD_OK ||
        mgcfd_mesh_level(mesh, 0, &desc) != MGCFD_OK)
        return fail("reading the wall nodes");
    std::vector<int64_t> ids(static_cast<size_t>(n));
    std::vector<double> table(static_cast<size_t>(n) * MGCFD_WALL_COLUMNS);
    if (n > 0 && mgcfd_wall_distribution(solver, 0, ids.data(), table.data()) != MGCFD_OK) return fail("computing the surface distribution");
    // --loads-heat: qw = h / area, T and St = qw / (rho_inf |V_inf| cp (T_total - Tw)) per node, Tw the held wall temperature or the node's own T
    std::vector<double> heat(conf.loads_heat ? static_cast<size_t>(n) * MGCFD_WALL_HEAT_COLUMNS : 0);
    double tw = 0.0, t_total = 0.0;
    bool isothermal = false;
    if (conf.loads_heat && ((n > 0 && mgcfd_wall_heat(solver, 0, nullptr, heat.data()) != MGCFD_OK) || wall_temperature_of(conf, ff17, &tw, &isothermal, &t_total) != MGCFD_OK))
        return fail("computing the wall heat table");
    const double vx = ff17[1] / ff17[0], vy = ff17[2] / ff17[0], vz = ff17[3] / ff17[0];
    const double q = 0.5 * ff17[0] * (vx * vx + vy * vy + vz * vz);
    std::string path = conf.output_file_prefix;
    if (!path.empty() && path.back() != '/') path += ".";
    path += "surface.size=" + std::to_string(conf.mesh_duplicate_count) + "x.level=0";
    FILE *f = std::fopen(path.c_str(), "w");
    if (!f) return fail(("opening " + path).c_str());
    std::fprintf(f, "node,x,y,z,ax,ay,az,Cp,Cfx,Cfy,Cfz%s\n", conf.loads_heat ? ",qw,T,St" : "");
    for (int64_t k = 0; k < n; k++) {
        const double *r = table.data() + static_cast<size_t>(k) * MGCFD_WALL_COLUMNS;
        const int64_t i = ids[static_cast<size_t>(k)];
        const double area = std::sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
        const double nx = r[0] / area, ny = r[1] / area, nz = r[2] / area;
        const double tn = r[4] * nx + r[5] * ny + r[6] * nz;
        const double cf[3] = {(r[4] - tn * nx) / (area * q), (r[5] - tn * ny) / (area * q), (r[6] - tn * nz) / (area * q)};
        std::fprintf(f, "%ld", static_cast<long>(i));
        for (int d = 0; d < 3; d++) std::fprintf(f, ",%.17e", desc.coords ? desc.coords[i * 3 + d] : 0.0);
        std::fprintf(f, ",%.17e,%.17e,%.17e,%.17e,%.17e,%.17e,%.17e", r[0], r[1], r[2], r[3] / q, cf[0], cf[1], cf[2]);
        if (conf.loads_heat) {
            const double *h = heat.data() + static_cast<size_t>(k) * MGCFD_WALL_HEAT_COLUMNS;
            const double qw = h[0] / h[2];
            std::fprintf(f, ",%.17e,%.17e,%.17e", qw, h[1], qw / (stanton_scale(ff17) * (t_total - (isothermal ? tw : h[1]))));
        }
        std::fprintf(f, "\n");
    }
    if (std::fclose(f) != 0) return fail(("writing " + path).c_str());
    return 0;
}

// --output-statistics: one row per node of level 0 in original order — id, coordinates, the means of rho u v w p mut, the resolved
// Reynolds stresses, p_rms and k (mgcfd_statistics_derive) — and a last comment line with the samples and the sum of their weights
int write_statistics_csv(const Config &conf, mgcfd_solver *solver, const mgcfd_mesh *mesh)
{
    int mode = 0;
    int64_t samples = 0;
    double wsum = 0.0;
    mgcfd_level_desc desc;
    if (mgcfd_get_statistics(solver, &mode, &samples, &wsum) != MGCFD_OK || mode == MGCFD_STATISTICS_OFF || mgcfd_mesh_level(mesh, 0, &desc) != MGCFD_OK)
        return fail("reading the flow statistics");
    const size_t nel = static_cast<size_t>(mgcfd_level_nel(solver, 0));
    std::vector<double> mean(nel * 6), mom(nel * 7), derived(nel * 8);
    if (mgcfd_get_array(solver, 0, MGCFD_ARR_STATISTICS_MEAN, mean.data()) != MGCFD_OK || mgcfd_get_array(solver, 0, MGCFD_ARR_STATISTICS_MOMENTS, mom.data()) != MGCFD_OK ||
        mgcfd_statistics_derive(wsum, mom.data(), static_cast<int64_t>(nel), derived.data()) != MGCFD_OK)
        return fail("reading the flow statistics");
    std::string path = conf.output_file_prefix;
    if (!path.empty() && path.back() != '/') path += ".";
    path += "statistics.size=" + std::to_string(conf.mesh_duplicate_count) + "x.level=0";
    FILE *f = std::fopen(path.c_str(), "w");
    if (!f) return fail(("opening " + path).c_str());
    std::fprintf(f, "node,x,y,z,rho,u,v,w,p,mut,Ruu,Rvv,Rww,Ruv,Ruw,Rvw,p_rms,k\n");
    for (size_t i = 0; i < nel; i++) {
        std::fprintf(f, "%ld", static_cast<long>(i));
        for (size_t d = 0; d < 3; d++) std::fprintf(f, ",%.17e", desc.coords ? desc.coords[i * 3 + d] : 0.0);
        for (size_t k = 0; k < 6; k++) std::fprintf(f, ",%.17e", mean[i * 6 + k]);
        for (size_t k = 0; k < 8; k++) std::fprintf(f, ",%.17e", derived[i * 8 + k]);
        std::fprintf(f, "\n");
    }
    std::fprintf(f, "# samples = %ld, wsum = %.17e\n", static_cast<long>(samples), wsum);
    if (std::fclose(f) != 0) return fail(("writing " + path).c_str());
    return 0;
}

// ... with --output-surface: one row per wall node of level 0 — id, coordinates, the mean Cp and the tangential mean Cf (write_surface_csv's
// expressions on the mean dp and t), the rms of Cp and, per component, the rms of t over |a| q_inf (the table holds no cross moments,
// so the fluctuation is not projected) — and the same last line
int write_surface_statistics_csv(const Config &conf, mgcfd_solver *solver, const mgcfd_mesh *mesh)
{
    int64_t n = 0, samples = 0;
    double ff17[17], wsum = 0.0;
    mgcfd_level_desc desc;
    if (mgcfd_wall_node_count(solver, 0, &n) != MGCFD_OK || mgcfd_get_far_field(solver, ff17) != MGCFD_OK || mgcfd_mesh_level(mesh, 0, &desc) != MGCFD_OK ||
        mgcfd_get_statistics(solver, nullptr, &samples, &wsum) != MGCFD_OK)
        return fail("reading the wall statistics");
    std::vector<int64_t> ids(static_cast<size_t>(n));
    std::vector<double> dist(static_cast<size_t>(n) * MGCFD_WALL_COLUMNS), table(static_cast<size_t>(n) * MGCFD_WALL_STATISTICS_COLUMNS);
    if (n > 0 && (mgcfd_wall_distribution(solver, 0, ids.data(), dist.data()) != MGCFD_OK || mgcfd_wall_statistics(solver, nullptr, table.data()) != MGCFD_OK))
        return fail("reading the wall statistics");
    const double vx = ff17[1] / ff17[0], vy = ff17[2] / ff17[0], vz = ff17[3] / ff17[0];
    const double q = 0.5 * ff17[0] * (vx * vx + vy * vy + vz * vz);
    std::string path = conf.output_file_prefix;
    if (!path.empty() && path.back() != '/') path += ".";
    path += "surface_statistics.size=" + std::to_string(conf.mesh_duplicate_count) + "x.level=0";
    FILE *f = std::fopen(path.c_str(), "w");
    if (!f) return fail(("opening " + path).c_str());
    std::fprintf(f, "node,x,y,z,Cp_mean,Cfx_mean,Cfy_mean,Cfz_mean,Cp_rms,Cfx_rms,Cfy_rms,Cfz_rms\n");
    for (int64_t k = 0; k < n; k++) {
        const double *a = dist.data() + static_cast<size_t>(k) * MGCFD_WALL_COLUMNS;
        const double *r = table.data() + static_cast<size_t>(k) * MGCFD_WALL_STATISTICS_COLUMNS;
        const int64_t i = ids[static_cast<size_t>(k)];
        const double area = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
        const double nx = a[0] / area, ny = a[1] / area, nz = a[2] / area;
        const double tn = r[1] * nx + r[2] * ny + r[3] * nz;
        std::fprintf(f, "%ld", static_cast<long>(i));
        for (int d = 0; d < 3; d++) std::fprintf(f, ",%.17e", desc.coords ? desc.coords[i * 3 + d] : 0.0);
        std::fprintf(f, ",%.17e,%.17e,%.17e,%.17e", r[0] / q, (r[1] - tn * nx) / (area * q), (r[2] - tn * ny) / (area * q), (r[3] - tn * nz) / (area * q));
        std::fprintf(f, ",%.17e", std::sqrt(r[4] / wsum) / q);
        for (int d = 0; d < 3; d++) std::fprintf(f, ",%.17e", std::sqrt(r[5 + d] / wsum) / (area * q));
        std::fprintf(f, "\n");
    }
    std::fprintf(f, "# samples = %ld, wsum = %.17e\n", static_cast<long>(samples), wsum);
    if (std::fclose(f) != 0) return fail(("writing " + path).c_str());
    return 0;
}

// The cycles of the whole run: without the free-stream options one batch, as ever; with them mgcfd_set_free_stream first
// (the first angle from its far field, a later angle of --polar from the flow before it) and one batch per angle.  rms and
// loads end up holding the LAST angle's histories.  set(mach, alpha, reinitialise) and cycles(rms, loads-or-null) return
// MGCFD codes.
template <typename Set, typename Cycles>
int run_all_cycles(const Config &conf, std::vector<double> &rms, std::vector<double> &loads, std::vector<PolarRow> &polar_rows,
                   Set &&set, Cycles &&cycles)
{
    const bool want_loads = conf.output_loads || conf.polar;
    if (!conf.free_stream_given && !conf.polar) return cycles(rms.data(), want_loads ? loads.data() : nullptr);
    for (int k = 0; k < conf.num_angles(); k++) {
        int rc = set(conf.ff_mach, conf.angle(k), k == 0 ? 1 : 0);
        if (rc != MGCFD_OK) return rc;
        rc = cycles(rms.data(), want_loads ? loads.data() : nullptr);
        if (rc != MGCFD_OK) return rc;
        if (conf.polar) {
            PolarRow row{};
            row.alpha = conf.angle(k); row.mach = conf.ff_mach;
            row.rms_last = rms.empty() ? std::nan("") : rms.back();
            for (size_t q = 0; q < conf.loads_width(); q++) row.loads[q] = loads.empty() ? std::nan("") : loads[loads.size() - conf.loads_width() + q];
            polar_rows.push_back(row);
        }
    }
    return MGCFD_OK;
}

// The viscosity of the run: --viscosity as given, or --reynolds against the free stream in use (the Mach number sets |V_inf|; the
// angle of attack does not change it, so a polar has one viscosity).
int viscosity_of(const Config &conf, double *mu)
{
    if (conf.viscosity_given) { *mu = conf.viscosity; return MGCFD_OK; }
    double ff17[17];
    const int rc = mgcfd_free_stream_constants(conf.ff_mach, conf.angle(0), ff17);
    return rc != MGCFD_OK ? rc : mgcfd_viscosity_from_reynolds(ff17, conf.reynolds, conf.ref_length, mu);
}

// Sutherland's reference of the run: --sutherland-tref as given, or p / rho of the free stream in use (the library's expression on
// its far field; the angle of attack does not change it)
int sutherland_tref_of(const Config &conf, double *t_ref)
{
    if (conf.sutherland_tref > 0.0) { *t_ref = conf.sutherland_tref; return MGCFD_OK; }
    double f[17];
    const int rc = mgcfd_free_stream_constants(conf.ff_mach, conf.angle(0), f);
    if (rc != MGCFD_OK) return rc;
    const double vx = f[1] / f[0], vy = f[2] / f[0], vz = f[3] / f[0];
    const double speed_sqd = vx * vx + vy * vy + vz * vz;
    *t_ref = ((1.4 - 1.0) * (f[4] - 0.5 * f[0] * speed_sqd)) / f[0];
    return MGCFD_OK;
}

// --gpus N (multi_gpu.cpp): the same outputs as the one-GPU run from N ranks of this process
int run_on_several_gpus(const Config &conf, mgcfd_mesh *mesh, int levels, int mesh_variant, int problem_size)
{
    try {
        multi_gpu::Options o;
        o.gpus = conf.gpus; o.first_device = conf.device; o.share_device = conf.gpus_share_device; o.fast_math = conf.fast_math;
        o.partition_levels = conf.gpus_partition;
        const auto tb = std::chrono::steady_clock::now();
        multi_gpu::Run run(mesh, o);
        std::fprintf(stderr, "[euler3d_gpu_double] %d ranks (%s), set up in %.2f s\n", run.ranks(),
                     run.partitioned_hierarchy() ? "every level partitioned, level 0 by recursive coordinate bisection; the V-cycle inside the library" :
                     run.partitioned() ? "level 0 partitioned by recursive coordinate bisection" : "one multigrid level per GPU",
                     std::chrono::duration<double>(std::chrono::steady_clock::now() - tb).count());
        std::vector<double> rms(static_cast<size_t>(conf.total_cycles()));
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<double> loads((conf.output_loads || conf.polar) ? static_cast<size_t>(conf.loads_rows()) * 6 : 0);
        std::vector<PolarRow> polar_rows;
        if (conf.time_step_given && run.set_time_step(conf.time_step_mode, conf.cfl) != MGCFD_OK) return fail("setting the time step");
        if (conf.smoothing_given && run.set_residual_smoothing(conf.smoothing_eps, conf.smoothing_iterations) != MGCFD_OK) return fail("setting the residual smoothing");
        if (conf.jst_given && run.set_jst(conf.jst_kappa2, conf.jst_kappa4, conf.jst_levels) != MGCFD_OK) return fail("setting the JST dissipation");
        if (conf.viscous()) {
            double mu = 0.0;
            if (viscosity_of(conf, &mu) != MGCFD_OK || run.set_viscous(mu, conf.prandtl, conf.no_slip ? 1 : 0, conf.viscous_cfl, conf.viscous_levels) != MGCFD_OK)
                return fail("setting the viscous terms");
        }
        const int rc = run_all_cycles(conf, rms, loads, polar_rows,
            [&](double mach, double alpha, int reinitialise) { return run.set_free_stream(mach, alpha, reinitialise); },
            [&](double *rms_out, double *loads_out) {
                // dual time stepping: switched on behind the free stream, so that the time levels start as the state
                if (conf.dual_given) {
                    const int rc_on = run.set_dual_time(conf.dual_dt, conf.dual_clamp, conf.bdf_order);
                    return rc_on != MGCFD_OK ? rc_on : run.advance(conf.time_steps, conf.num_cycles, rms_out);
                }
                return loads_out ? run.run_cycles_loads(conf.num_cycles, conf.loads_ref + 2, rms_out, loads_out) : run.run_cycles(conf.num_cycles, rms_out);
            });
        for (PolarRow &row : polar_rows) {          // (the coefficients of an angle are taken against that angle's far field)
            if (mgcfd_free_stream_constants(row.mach, row.alpha, row.ff17) != MGCFD_OK) return fail("the free stream of a polar row");
        }
        const double total_compute_time = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        for (int i = 0; i < conf.total_cycles(); i++)
            std::printf(levels <= 1 ? "\nCycle %d / %d (RMS = %.3e)" : "\nMG cycle %d / %d (RMS = %.3e)", i + 1, conf.total_cycles(), rms[static_cast<size_t>(i)]);
        std::printf("\n");
        if (rc == MGCFD_ERR_NAN || rc == MGCFD_ERR_NEG_DENSITY || rc == MGCFD_ERR_NEG_ENERGY) {
            std::printf(rc == MGCFD_ERR_NAN ? "\nERROR: NaN detected!\n" : rc == MGCFD_ERR_NEG_DENSITY ? "\nERROR: Negative density detected!\n" : "\nERROR: Negative density.energy detected!\n");
            return EXIT_FAILURE;
        }
        if (rc != MGCFD_OK) return fail("running the cycles");
        std::printf("Total runtime = %g\n", total_compute_time);
        mgcfd_level_desc d0;
        mgcfd_mesh_level(mesh, 0, &d0);
        // -v and every dump as on one GPU (level 0 gathered from the ranks that own its nodes)
        if (validate_and_dump(conf, levels, mesh_variant, d0.nel,
                              [&](int which, int ncols, double *out) { run.get_level0(which, ncols, out); return MGCFD_OK; },
                              [&](int level, int64_t *bad) { return run.check_invalid(level, bad); }))
            return EXIT_FAILURE;
        if (conf.output_loads) {
            double ff17[17];
            run.far_field(ff17);
            if (write_loads_csv(conf, ff17, loads)) return EXIT_FAILURE;
        }
        if (conf.polar && write_polar_csv(conf, polar_rows)) return EXIT_FAILURE;
        std::string device_name = "unknown GPU";
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, conf.device) == hipSuccess) device_name = prop.name;
        std::string ih, il;
        csv_identification(conf, problem_size, mesh_variant, device_name, ih, il, run.ranks());
        std::vector<std::vector<std::string>> times(static_cast<size_t>(levels)), iters(static_cast<size_t>(levels));
        for (int l = 0; l < levels; l++) {
            int64_t n[MGCFD_NUM_LOOPS];
            run.loop_iters(l, conf.total_cycles() * conf.num_angles(), n);
            for (int k = 0; k < MGCFD_NUM_LOOPS; k++) { times[static_cast<size_t>(l)].push_back("0"); iters[static_cast<size_t>(l)].push_back(std::to_string(n[k])); }
        }
        const std::string tpath = csv_filepath(conf, "Times.csv"), ipath = csv_filepath(conf, "LoopNumIters.csv");
        write_csv(tpath, ih, il, levels, times, true, total_compute_time);
        std::printf("Loop runtimes written to: %s\n", tpath.c_str());
        write_csv(ipath, ih, il, levels, iters, false, 0.0);
        std::printf("Loop stats written to: %s\n", ipath.c_str());
        return 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "ERROR: %s\n", e.what());
        return EXIT_FAILURE;
    }
}

} // namespace

int main(int argc, char **argv)
{
    const double epoch_at_main = std::chrono::duration<double>(std::chrono::system_clock::now().time_since_epoch()).count();
    Config conf;
    if (!parse_arguments(argc, argv, conf)) return 1;
    if (conf.output_loads && conf.gpus > 1 && !conf.gpus_partition) {
        std::fprintf(stderr, "ERROR: --output-loads runs on one GPU only, or on --gpus N with --gpus-partition (every level split over the ranks)\n");
        return 1;
    }
    if (conf.smoothing_given && conf.smoothing_iterations > 0 && conf.gpus > 1 && conf.gpus_partition) {
        std::fprintf(stderr, "ERROR: residual smoothing (--residual-smoothing) does not run with --gpus-partition: a level split over GPUs would need a halo exchange per Jacobi iteration\n");
        return 1;
    }
    if (conf.jst_given && conf.jst_levels > 0 && conf.gpus > 1 && conf.gpus_partition) {
        std::fprintf(stderr, "ERROR: the JST dissipation (--jst) does not run with --gpus-partition: a level split over GPUs would need its sensor and Laplacian exchanged per stage\n");
        return 1;
    }
    if (conf.viscous() && conf.viscous_levels > 0 && conf.gpus > 1 && conf.gpus_partition) {
        std::fprintf(stderr, "ERROR: the viscous terms (--viscosity, --reynolds) do not run with --gpus-partition: a level split over GPUs would need its node stresses exchanged per stage\n");
        return 1;
    }
    if (conf.dual_given && conf.gpus > 1 && conf.gpus_partition) {
        std::fprintf(stderr, "ERROR: dual time stepping (--physical-time-step) does not run with --gpus-partition: levels split over GPUs are out of scope\n");
        return 1;
    }
    if (conf.fas && conf.gpus > 1) {
        std::fprintf(stderr, "ERROR: FAS multigrid (--fas) runs on one GPU only: levels split over GPUs, or one level per GPU, would need the residuals, the forcing and the corrections exchanged\n");
        return 1;
    }
    if ((conf.cycle_given() || !conf.fmg_cycles.empty()) && conf.gpus > 1) {
        std::fprintf(stderr, "ERROR: --cycle, --pre-sweeps, --post-sweeps and --fmg-cycles run on one GPU only: levels split over GPUs, or one level per GPU, run the default cycle\n");
        return 1;
    }
    if (!conf.fmg_cycles.empty() && (conf.dual_given || conf.polar)) {
        std::fprintf(stderr, "ERROR: a full-multigrid start (--fmg-cycles) does not run with --physical-time-step or --polar\n");
        return 1;
    }
    if (conf.dual_given && conf.polar) {
        std::fprintf(stderr, "ERROR: dual time stepping (--physical-time-step) does not run with --polar\n");
        return 1;
    }
    if (conf.polar && conf.gpus > 1 && !conf.gpus_partition) {
        std::fprintf(stderr, "ERROR: --polar runs on one GPU only, or on --gpus N with --gpus-partition (every level split over the ranks)\n");
        return 1;
    }
    if (conf.free_stream_given || conf.polar) {
        // (the arguments are checked before any file is read: the same rule as mgcfd_set_free_stream's)
        double ff17[17];
        for (int k = 0; k < conf.num_angles(); k += std::max(1, conf.num_angles() - 1))
            if (mgcfd_free_stream_constants(conf.ff_mach, conf.angle(k), ff17) != MGCFD_OK) {
                std::fprintf(stderr, "ERROR: %s\n", mgcfd_last_error());
                return 1;
            }
    }
    if (conf.input_file.empty()) {
        std::printf("ERROR: input_file not set\n");
        return 1;
    }

    const auto t_start = std::chrono::steady_clock::now();
    // (a reconstructing run first learns whether its levels came with coordinates: no GPU work before that)
    const bool needs_coords = conf.upwind_given && conf.upwind_levels > 0 && conf.muscl_levels() > 0;
    if (conf.gpus <= 1 && !needs_coords) mgcfd_device_warm_up(conf.device);      // (the runtime comes up while the files are read)
    mgcfd_mesh *mesh = nullptr;
    if (mgcfd_mesh_load_ex(conf.input_file.c_str(), conf.input_file_directory.c_str(), conf.mesh_duplicate_count,
                           conf.legacy_ordering ? MGCFD_MESH_LEGACY_ORDERING : 0, &mesh) != MGCFD_OK)
        return fail("reading input");
    const int levels = mgcfd_mesh_num_levels(mesh);
    const int mesh_variant = mgcfd_mesh_variant(mesh);
    const int problem_size = mgcfd_mesh_size(mesh);

    const double t_read = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
    if (needs_coords)
        for (int l = 0; l < levels && l < conf.muscl_levels(); l++) {
            mgcfd_level_desc d;
            if (mgcfd_mesh_level(mesh, l, &d) != MGCFD_OK) return fail("reading input");
            if (!d.coords) {
                std::fprintf(stderr, "ERROR: the upwind flux (--upwind) reconstructs on level %d, whose coords were not read (no .coords file, or a single-level fvcorr input, which reads none): give --muscl-levels %d\n", l, l);
                return 1;
            }
        }
    if (conf.fas && levels < 2) {
        std::fprintf(stderr, "ERROR: FAS multigrid (--fas) needs an input of two levels or more: with one level there is no coarse level to force and no correction to bring back\n");
        return 1;
    }
    // the lists of the cycle flags, one entry per level
    std::vector<int> pre(static_cast<size_t>(levels), 1), post(static_cast<size_t>(levels), 1), fmg(static_cast<size_t>(levels), 0);
    post[0] = 0;
    {
        const size_t n = static_cast<size_t>(levels);
        if (conf.pre_sweeps.size() == 1) pre.assign(n, conf.pre_sweeps[0]);
        else if (conf.pre_sweeps.size() == n) pre = conf.pre_sweeps;
        else if (!conf.pre_sweeps.empty()) { std::fprintf(stderr, "ERROR: --pre-sweeps: one value, or one per level (%d)\n", levels); return 1; }
        if (conf.post_sweeps.size() == 1) std::fill(post.begin(), post.end() - 1, conf.post_sweeps[0]);      // (the coarsest level is left alone)
        else if (conf.post_sweeps.size() == n) post = conf.post_sweeps;
        else if (!conf.post_sweeps.empty()) { std::fprintf(stderr, "ERROR: --post-sweeps: one value, or one per level (%d)\n", levels); return 1; }
        if (conf.fmg_cycles.size() == 1) std::fill(fmg.begin() + 1, fmg.end(), conf.fmg_cycles[0]);
        else if (conf.fmg_cycles.size() + 1 == n) std::copy(conf.fmg_cycles.begin(), conf.fmg_cycles.end(), fmg.begin() + 1);
        else if (!conf.fmg_cycles.empty()) { std::fprintf(stderr, "ERROR: --fmg-cycles: one value, or one per level 1 ... %d\n", levels - 1); return 1; }
    }
    if (conf.gpus > 1) return run_on_several_gpus(conf, mesh, levels, mesh_variant, problem_size);

    mgcfd_solver *solver = nullptr;
    const auto t_create = std::chrono::steady_clock::now();
    if (mgcfd_create_from_mesh(mesh, conf.device, &solver) != MGCFD_OK) return fail("creating the GPU solver");
    // where the wall time outside the reference's timed region goes (stderr: stdout stays the reference's, line for line)
    std::fprintf(stderr, "[euler3d_gpu_double] input files read in %.2f s, gather plans built and uploaded in %.2f s\n", t_read,
                 std::chrono::duration<double>(std::chrono::steady_clock::now() - t_create).count());
    const auto t_created = std::chrono::steady_clock::now();
    mgcfd_set_option(solver, MGCFD_OPT_EXACT, conf.fast_math ? 0 : 1);
    mgcfd_set_option(solver, MGCFD_OPT_TIMING, conf.timers ? (conf.loop_timers ? 1 : 4) : 0);
    mgcfd_set_option(solver, MGCFD_OPT_INDIRECT_RW, (conf.indirect_rw && conf.timers) ? 1 : 0);

    std::string device_name = "unknown GPU";
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, conf.device) == hipSuccess) device_name = prop.name;
    }

    // ---- compute (src/euler3d_cpu_double.cpp:368-698) ----
    std::vector<double> rms(static_cast<size_t>(conf.total_cycles()));
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<double> loads((conf.output_loads || conf.polar) ? static_cast<size_t>(conf.loads_rows()) * conf.loads_width() : 0);
    int steps_done = 0;               // dual time stepping: physical steps completed (an invalid state: the step it was found in)
    std::vector<PolarRow> polar_rows;
    if (conf.time_step_given && mgcfd_set_time_step(solver, conf.time_step_mode, conf.cfl) != MGCFD_OK) return fail("setting the time step");
    if (conf.smoothing_given && mgcfd_set_residual_smoothing(solver, conf.smoothing_eps, conf.smoothing_iterations) != MGCFD_OK) return fail("setting the residual smoothing");
    if (conf.jst_given && mgcfd_set_jst(solver, conf.jst_kappa2, conf.jst_kappa4, conf.jst_levels) != MGCFD_OK) return fail("setting the JST dissipation");
    if (conf.upwind_given && mgcfd_set_upwind(solver, conf.upwind_levels, conf.muscl_levels(), conf.limiter, conf.venkat_k, conf.entropy_fix) != MGCFD_OK)
        return fail("setting the upwind flux");
    if (conf.viscous()) {
        double mu = 0.0;
        if (conf.face_gradient_given && mgcfd_set_face_gradient(solver, conf.face_gradient) != MGCFD_OK) return fail("setting the face gradient");
        if (viscosity_of(conf, &mu) != MGCFD_OK || mgcfd_set_viscous(solver, mu, conf.prandtl, conf.no_slip ? 1 : 0, conf.viscous_cfl, conf.viscous_levels) != MGCFD_OK)
            return fail("setting the viscous terms");
        double t_ref = 0.0;
        if (conf.viscosity_model() && sutherland_tref_of(conf, &t_ref) != MGCFD_OK) return fail("setting the viscosity model");
        if (conf.spalart_allmaras && mgcfd_set_sa_free_stream(solver, conf.sa_ratio, 0) != MGCFD_OK) return fail("setting the Spalart-Allmaras free stream");
        if (conf.sa_unsteady_given && mgcfd_set_sa_unsteady(solver, conf.sa_time_accurate ? 1 : 0, conf.sa_length, conf.sa_cdes) != MGCFD_OK)
            return fail("setting the unsteady Spalart-Allmaras model");
        if (conf.viscosity_model() &&
            mgcfd_set_viscosity_model(solver, conf.sutherland ? MGCFD_VISCOSITY_SUTHERLAND : MGCFD_VISCOSITY_CONSTANT, t_ref, conf.sutherland_s,
                                      conf.spalart_allmaras ? MGCFD_EDDY_SPALART_ALLMARAS : (conf.smagorinsky ? MGCFD_EDDY_SMAGORINSKY : MGCFD_EDDY_NONE),
                                      conf.smagorinsky_cs, conf.prandtl_turbulent) != MGCFD_OK)
            return fail("setting the viscosity model");
        if (conf.wall_damping && mgcfd_set_wall_damping(solver, 1, conf.wall_kappa) != MGCFD_OK) return fail("setting the wall damping");
        if (conf.wall_thermal_flags > 0) {
            // (the ratio against the free stream in use after --mach / --alpha; the angle of attack does not change its temperature)
            double f[17], t_static = 0.0;
            if (mgcfd_free_stream_constants(conf.ff_mach, conf.angle(0), f) != MGCFD_OK || mgcfd_free_stream_temperature(f, &t_static, nullptr) != MGCFD_OK ||
                mgcfd_set_wall_temperature(solver, conf.wall_mode, conf.wall_ratio ? conf.wall_value * t_static : conf.wall_value) != MGCFD_OK)
                return fail("setting the wall thermal condition");
        }
    }
    if (conf.fas && mgcfd_set_fas(solver, 1) != MGCFD_OK) return fail("switching FAS multigrid on");
    if (conf.cycle_given() && mgcfd_set_cycle(solver, conf.cycle_shape, pre.data(), post.data()) != MGCFD_OK) return fail("setting the multigrid cycle");
    const int rc = run_all_cycles(conf, rms, loads, polar_rows,
        [&](double mach, double alpha, int reinitialise) { return mgcfd_set_free_stream(solver, mach, alpha, reinitialise); },
        [&](double *rms_out, double *loads_out) {
            if (conf.dual_given) {
                // switched on behind the free stream, so that the time levels start as the state; mgcfd_advance takes at most
                // MGCFD_MAX_ADVANCE_CYCLES cycles per call: whole physical steps per call
                int rc_on = mgcfd_set_dual_time(solver, conf.dual_dt, conf.dual_clamp);
                if (rc_on == MGCFD_OK) rc_on = mgcfd_dual_time_set_order(solver, conf.bdf_order);
                if (rc_on != MGCFD_OK) return rc_on;
                const int per_call = std::max(1, MGCFD_MAX_ADVANCE_CYCLES / conf.num_cycles);
                for (steps_done = 0; steps_done < conf.time_steps;) {
                    int now = std::min(per_call, conf.time_steps - steps_done);
                    // --output-statistics: a call ends where the sampling begins, and the statistics go on behind it
                    if (conf.output_statistics && steps_done < conf.statistics_start) now = std::min(now, conf.statistics_start - steps_done);
                    if (conf.output_statistics && steps_done == conf.statistics_start) {
                        const int rc_st = mgcfd_set_statistics(solver, conf.output_surface ? MGCFD_STATISTICS_VOLUME_AND_WALL : MGCFD_STATISTICS_VOLUME);
                        if (rc_st != MGCFD_OK) return rc_st;
                    }
                    double *const rms_at = rms_out + size_t(steps_done) * size_t(conf.num_cycles);
                    double *const loads_at = loads_out ? loads_out + size_t(steps_done) * conf.loads_width() : nullptr;
                    const int rc_adv = conf.loads_heat && loads_at ? mgcfd_advance_loads_heat(solver, now, conf.num_cycles, rms_at, loads_at, conf.loads_ref + 2)
                                     : conf.loads_friction ? mgcfd_advance_loads_viscous(solver, now, conf.num_cycles, rms_at, loads_at, conf.loads_ref + 2)
                                                           : mgcfd_advance(solver, now, conf.num_cycles, rms_at, loads_at, conf.loads_ref + 2);
                    if (rc_adv != MGCFD_OK) {
                        int bad_step = -1;
                        mgcfd_get_dual_time(solver, nullptr, nullptr, nullptr, nullptr, &bad_step);
                        if (bad_step >= 0) steps_done += bad_step;
                        return rc_adv;
                    }
                    steps_done += now;
                }
                return int(MGCFD_OK);
            }
            if (!conf.fmg_cycles.empty()) {
                // the full-multigrid start, behind the free stream: its histories go to stderr (stdout stays the reference's lines)
                std::vector<double> fmg_rms(static_cast<size_t>(std::max(1, std::accumulate(fmg.begin() + 1, fmg.end(), 0))));
                const int rc_fmg = mgcfd_full_multigrid(solver, fmg.data(), fmg_rms.data());
                if (rc_fmg != MGCFD_OK) return rc_fmg;
                size_t at = 0;
                for (int top = levels - 1; top >= 1; at += static_cast<size_t>(fmg[static_cast<size_t>(top)]), top--)
                    if (fmg[static_cast<size_t>(top)] > 0)
                        std::fprintf(stderr, "[euler3d_gpu_double] full multigrid: %d cycles from level %d, RMS %.3e -> %.3e\n", fmg[static_cast<size_t>(top)], top,
                                     fmg_rms[at], fmg_rms[at + static_cast<size_t>(fmg[static_cast<size_t>(top)]) - 1]);
            }
            if (loads_out && conf.loads_heat) return mgcfd_run_cycles_loads_heat(solver, conf.num_cycles, conf.loads_ref + 2, rms_out, loads_out);
            if (loads_out && conf.loads_friction) return mgcfd_run_cycles_loads_viscous(solver, conf.num_cycles, conf.loads_ref + 2, rms_out, loads_out);
            return loads_out ? mgcfd_run_cycles_loads(solver, conf.num_cycles, conf.loads_ref + 2, rms_out, loads_out)
                             : mgcfd_run_cycles(solver, conf.num_cycles, rms_out);
        });
    for (PolarRow &row : polar_rows)            // (the coefficients of an angle are taken against that angle's far field)
        if (mgcfd_free_stream_constants(row.mach, row.alpha, row.ff17) != MGCFD_OK) return fail("the free stream of a polar row");
    const double total_compute_time = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    const bool invalid = rc == MGCFD_ERR_NAN || rc == MGCFD_ERR_NEG_DENSITY || rc == MGCFD_ERR_NEG_ENERGY;
    int64_t bad_cell = -1;
    int bad_cycle = -1;
    if (invalid) mgcfd_invalid_state_location(solver, &bad_cell, &bad_cycle);
    // (the reference prints a cycle's line when the cycle starts and exits inside the failing time_step)
    if (invalid && bad_cycle >= 0 && conf.dual_given) bad_cycle += steps_done * conf.num_cycles;      // (counted through the physical steps)
    const int printed = invalid && bad_cycle >= 0 ? bad_cycle + 1 : conf.total_cycles();
    for (int i = 0; i < printed; i++) {
        std::printf(levels <= 1 ? "\nCycle %d / %d" : "\nMG cycle %d / %d", i + 1, conf.total_cycles());
        if (!(invalid && i == bad_cycle)) std::printf(" (RMS = %.3e)", rms[static_cast<size_t>(i)]);
    }
    std::printf("\n");
    if (invalid) {
        // check_for_invalid_variables' messages (src/Kernels/validation.cpp:112-134); the cell's values at that
        // moment are not kept on the device
        std::printf(rc == MGCFD_ERR_NAN ? "\nERROR: NaN detected!" :
                    rc == MGCFD_ERR_NEG_DENSITY ? "\nERROR: Negative density detected!" : "\nERROR: Negative density.energy detected!");
        std::printf("\nCell %ld\n", static_cast<long>(bad_cell));
        return EXIT_FAILURE;
    }
    if (rc != MGCFD_OK) return fail("running the cycles");
    std::printf("Total runtime = %g\n", total_compute_time);

    const int64_t nel0 = mgcfd_level_nel(solver, 0);
    // ---- validate, dumps (src/euler3d_cpu_double.cpp:704-772) ----
    if (validate_and_dump(conf, levels, mesh_variant, nel0,
                          [&](int which, int ncols, double *out) { (void)ncols; return mgcfd_get_array(solver, 0, which, out); },
                          [&](int level, int64_t *bad) { return mgcfd_check_for_invalid_variables(solver, level, bad); }))
        return EXIT_FAILURE;
    if (conf.output_loads) {
        double ff17[17];
        if (mgcfd_get_far_field(solver, ff17) != MGCFD_OK) return fail("reading the far field");
        if (write_loads_csv(conf, ff17, loads)) return EXIT_FAILURE;
    }
    if (conf.polar && write_polar_csv(conf, polar_rows)) return EXIT_FAILURE;
    if (conf.output_surface && write_surface_csv(conf, solver, mesh)) return EXIT_FAILURE;
    if (conf.output_statistics && write_statistics_csv(conf, solver, mesh)) return EXIT_FAILURE;
    if (conf.output_statistics && conf.output_surface && write_surface_statistics_csv(conf, solver, mesh)) return EXIT_FAILURE;

    // ---- performance data (src/euler3d_cpu_double.cpp:778-785) ----
    std::string ih, il;
    csv_identification(conf, problem_size, mesh_variant, device_name, ih, il);
    std::vector<std::vector<std::string>> times(static_cast<size_t>(levels)), iters(static_cast<size_t>(levels));
    for (int l = 0; l < levels; l++) {
        double t[MGCFD_NUM_LOOPS];
        int64_t n[MGCFD_NUM_LOOPS];
        mgcfd_get_loop_times(solver, l, t);
        mgcfd_get_loop_iters(solver, l, n);
        for (int k = 0; k < MGCFD_NUM_LOOPS; k++) {
            std::ostringstream a, b;
            a << t[k];
            b << n[k];
            times[static_cast<size_t>(l)].push_back(a.str());
            iters[static_cast<size_t>(l)].push_back(b.str());
        }
    }
    const std::string tpath = csv_filepath(conf, "Times.csv"), ipath = csv_filepath(conf, "LoopNumIters.csv");
    write_csv(tpath, ih, il, levels, times, true, total_compute_time);
    std::printf("Loop runtimes written to: %s\n", tpath.c_str());
    write_csv(ipath, ih, il, levels, iters, false, 0.0);
    std::printf("Loop stats written to: %s\n", ipath.c_str());

    const auto t_out = std::chrono::steady_clock::now();
    mgcfd_destroy(solver);
    mgcfd_mesh_free(mesh);
    if (std::getenv("MGCFD_PLAN_TIMING"))       // (the two epoch times let a caller see what the process spends before main() and after it)
        std::fprintf(stderr, "[euler3d_gpu_double] main() began at %.3f and returns at %.3f (seconds of the epoch)\n", epoch_at_main,
                     std::chrono::duration<double>(std::chrono::system_clock::now().time_since_epoch()).count());
    if (std::getenv("MGCFD_PLAN_TIMING"))
        std::fprintf(stderr, "[euler3d_gpu_double] since main() began: files read %.3f s, solver created %.3f s, cycles done %.3f s, outputs written %.3f s, freed %.3f s\n",
                     t_read, std::chrono::duration<double>(t_created - t_start).count(), std::chrono::duration<double>(t0 - t_start).count() + total_compute_time,
                     std::chrono::duration<double>(t_out - t_start).count(), std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count());
    return 0;
}
