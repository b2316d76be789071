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

// What the run was asked for.  Which flag or config key sets which field, and how its value is read: kOptions, below.
struct Config {                       // the reference's `config` (src/Base/config.h:27-47)
    std::string config_filepath, input_file, input_file_directory, papi_config_file, output_file_prefix;
    int mesh_duplicate_count = 1;
    int num_cycles = 25;              // src/Base/config.cpp:63
    bool validate_result = false;
    bool output_variables = false, output_old_variables = false, output_step_factors = false,
         output_edge_fluxes = false, output_fluxes = false, output_volumes = false;
    // extensions (not in the reference)
    bool timers = true;               // off: fused fast path (one launch per Runge-Kutta stage); Times.csv holds only Total
    bool loop_timers = false;         // EVERY loop its own launch between two events, as the reference's -DTIME build brackets
                                      // them (src/Monitoring/timer.cpp:58-195); default: fused stages, the per-loop times ATTRIBUTED
                                      // from every 32nd sweep / transfer of a level, which runs per loop under events (MGCFD_OPT_TIMING = 4)
    bool fast_math = false;           // allow FMA contraction (MGCFD_OPT_EXACT = 0)
    bool indirect_rw = true;          // the reference runs the probe every RK stage
    bool legacy_ordering = false;     // the reference's -DLEGACY_ORDERING edge sort (a compile-time flag there)
    int device = 0;
    int gpus = 1;                     // N: a single-level input partitioned over N GPUs, a multigrid input one level per GPU
    bool gpus_share_device = false;   // all N ranks on the one device (rehearsal on a one-GPU box)
    bool gpus_partition = false;      // split every level of a multigrid input over the N GPUs (the default when N > levels)
    bool output_loads = false;        // the level-0 surface loads of every cycle into surface_loads.*
    double loads_ref[5] = {1.0, 1.0, 0.0, 0.0, 0.0};   // S,c,x,y,z: reference area, length and moment point
    // the free stream (the reference compiles it in: ff_mach = 1.2, deg_angle_of_attack = 0, src/Base/const.h:14-15)
    bool free_stream_given = false;   // mgcfd_set_free_stream before the first cycle
    double ff_mach = 1.2, angle_of_attack = 0.0;
    bool polar = false;               // polar_n angles from polar_a0 to polar_a1 inclusive, num_cycles each, polar.csv
    double polar_a0 = 0.0, polar_a1 = 0.0;
    int polar_n = 0;
    // the time step (the reference ties it to the mesh name and the literal 0.5, src/euler3d_cpu_double.cpp:388-395)
    bool time_step_given = false;     // mgcfd_set_time_step before the first cycle
    int time_step_mode = MGCFD_DT_REFERENCE;
    double cfl = 0.5;
    bool config_bad = false;          // a config file's value was refused: the run ends right after parsing
    // implicit residual smoothing
    bool smoothing_given = false;     // an EPS was given: mgcfd_set_residual_smoothing before the first cycle
    bool smoothing_iterations_given = false;
    double smoothing_eps = 0.0;
    int smoothing_iterations = 2;     // (the default when only EPS is given)
    // JST dissipation; each of its three values switches it on
    bool jst_given = false;           // mgcfd_set_jst before the first cycle
    double jst_kappa2 = MGCFD_JST_KAPPA2, jst_kappa4 = MGCFD_JST_KAPPA4;
    int jst_levels = 1;
    // upwind fluxes; each of their five values switches them on
    bool upwind_given = false;        // mgcfd_set_upwind before the first cycle
    int upwind_levels = 1, muscl_levels_said = -1, limiter = MGCFD_LIMITER_VENKATAKRISHNAN;
    double venkat_k = MGCFD_UPWIND_VENKAT_K, entropy_fix = MGCFD_UPWIND_ENTROPY_FIX;
    int muscl_levels() const { return muscl_levels_said < 0 ? upwind_levels : muscl_levels_said; }   // (not said: every upwind level reconstructs)
    // laminar viscous terms
    bool viscosity_given = false, reynolds_given = false;   // one of the two switches the terms on: mgcfd_set_viscous before the first cycle
    bool viscous_extras_given = false;                      // one of the companions was given (they need MU or RE)
    double viscosity = 0.0, reynolds = 0.0, ref_length = 1.0, prandtl = MGCFD_VISCOUS_PRANDTL, viscous_cfl = MGCFD_VISCOUS_CFL;
    bool no_slip = false;
    int viscous_levels = 1;
    bool viscous() const { return viscosity_given || reynolds_given; }
    // the viscosity model: Sutherland's law, and the Smagorinsky or Spalart-Allmaras eddy viscosity
    bool sutherland = false, smagorinsky = false;
    bool model_extras_given = false;                        // a companion of the models was given (they need the viscous terms)
    double sutherland_tref = 0.0, sutherland_s = MGCFD_SUTHERLAND_S, smagorinsky_cs = MGCFD_SMAGORINSKY_CS, prandtl_turbulent = MGCFD_PRANDTL_TURBULENT;
    bool viscosity_model() const { return sutherland || smagorinsky || spalart_allmaras; }
    bool spalart_allmaras = false;    // the transported eddy viscosity (MGCFD_EDDY_SPALART_ALLMARAS)
    double sa_ratio = MGCFD_SA_RATIO; // the free-stream nu_tilde over nu (mgcfd_set_sa_free_stream)
    // the unsteady Spalart-Allmaras model (mgcfd_set_sa_unsteady); time-accurate, it runs under dual time stepping
    bool sa_time_accurate = false, sa_unsteady_given = false;
    int sa_length = MGCFD_SA_LENGTH_WALL;
    double sa_cdes = MGCFD_SA_CDES;
    bool wall_damping = false;        // the wall-limited length scale of the Smagorinsky model (mgcfd_set_wall_damping)
    double wall_kappa = MGCFD_WALL_KAPPA;
    bool loads_friction = false;      // the friction loads beside the pressure loads in surface_loads.* and polar.csv
    bool output_surface = false;      // Cp and Cf per wall node of level 0 into surface.*
    // wall thermal conditions (mgcfd_set_wall_temperature): a temperature, a ratio to the static free-stream temperature in use,
    // or a heat flux; one of them at most
    int wall_thermal_flags = 0;       // how many of the three were given
    int wall_mode = 0;                // MGCFD_WALL_*
    double wall_value = 0.0;          // T, R or Q as given
    bool wall_ratio = false;          // ... it is R
    // the face gradient of the viscous and Spalart-Allmaras diffusion (mgcfd_set_face_gradient).  Corrected, and no viscous_cfl
    // given: MGCFD_VISCOUS_CFL_CORRECTED
    int face_gradient = MGCFD_FACE_GRADIENT_AVERAGED;
    bool face_gradient_given = false, viscous_cfl_given = false;
    bool loads_heat = false;          // Q, A and the mean Stanton number behind the friction columns; qw, T, St in surface.*
    size_t loads_width() const { return loads_heat ? 14 : (loads_friction ? 12 : 6); }
    bool fas = false;                 // FAS multigrid: mgcfd_set_fas before the first cycle
    // the multigrid cycle (mgcfd_set_cycle before the first cycle) and the full-multigrid start (mgcfd_full_multigrid before the
    // cycles); the lists are expanded once the number of levels is known
    int cycle_shape = MGCFD_CYCLE_V;
    std::vector<int> pre_sweeps, post_sweeps, fmg_cycles;
    bool cycle_given() const { return cycle_shape != MGCFD_CYCLE_V || !pre_sweeps.empty() || !post_sweeps.empty(); }
    // dual time stepping.  With DT given, num_cycles is the number of cycles per physical step.
    bool dual_given = false;          // a DT was given: mgcfd_set_dual_time before the first cycle, mgcfd_advance for the cycles
    bool dual_extras_given = false;   // one of the three companions was given (they need DT)
    double dual_dt = 0.0, dual_clamp = MGCFD_DUAL_TIME_CLAMP;
    int time_steps = 1, bdf_order = 2;
    // flow statistics (mgcfd_set_statistics): statistics.* (and, with output_surface, surface_statistics.*) from the samples
    // mgcfd_advance takes; the first statistics_start physical steps are not sampled
    bool output_statistics = false, statistics_start_given = false;
    int statistics_start = 0;
    int steps() const { return dual_given ? time_steps : 1; }
    int total_cycles() const { return (num_cycles > 0 ? num_cycles : 0) * steps(); }      // RMS lines of the run
    int loads_rows() const { return dual_given ? time_steps : (num_cycles > 0 ? num_cycles : 0); }   // one row per physical step
    // the k-th angle of the run (one angle without a polar)
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
// a finite number above zero
bool parse_positive(const char *text, double *out)
{
    double v = 0.0;
    if (!parse_number(text, &v) || !(v > 0.0)) return false;
    *out = v;
    return true;
}
// a finite number not below zero
bool parse_not_negative(const char *text, double *out)
{
    double v = 0.0;
    if (!parse_number(text, &v) || !(v >= 0.0)) return false;
    *out = v;
    return true;
}
// a whole number lo ... hi
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

// ---- the options that need more than a kind of value: each a function of its own, named by its entry in kOptions

// --polar "A0:A1:N": two finite angles and a count of at least 1
bool set_polar(Config &c, const char *text)
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

// --loads-reference "S,c,x,y,z": five finite numbers, S and c positive; false on anything else
bool set_loads_reference(Config &c, const char *text)
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
        c.loads_ref[k] = v;
        p = end;
    }
    return *p == '\0' && c.loads_ref[0] > 0.0 && c.loads_ref[1] > 0.0;
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
bool set_wall_temperature(Config &c, const char *text) { return set_wall_thermal(c, 0, text); }
bool set_wall_temperature_ratio(Config &c, const char *text) { return set_wall_thermal(c, 1, text); }
bool set_wall_heat_flux(Config &c, const char *text) { return set_wall_thermal(c, 2, text); }

bool set_no_slip(Config &c, const char *) { return c.no_slip = c.viscous_extras_given = true; }
bool set_sa_time_accurate(Config &c, const char *) { return c.sa_time_accurate = c.sa_unsteady_given = true; }
bool set_viscous_cfl(Config &c, const char *text)
{
    if (!parse_positive(text, &c.viscous_cfl)) return false;
    return c.viscous_extras_given = c.viscous_cfl_given = true;
}
// --entropy-fix: Harten's fraction, 0 ... 1
bool set_entropy_fix(Config &c, const char *text)
{
    if (!parse_not_negative(text, &c.entropy_fix) || c.entropy_fix > 1.0) return false;
    return c.upwind_given = true;
}
void read_config(Config &c);
// -c: the file is read where it stands among the arguments, so an argument behind it overrides the file's value
bool set_config_filepath(Config &c, const char *text)
{
    c.config_filepath = text;
    read_config(c);
    return true;
}
void print_help();
// -h: refuses without a phrase, which ends the parsing without an error message
bool help_and_stop(Config &, const char *)
{
    print_help();
    return false;
}

// ---- the option table: every flag of the command line and every key of a config file, once

enum class Read {
    Flag,          // sets its bool (a config file: by the value Y only)
    FlagOff,       // clears its bool
    String,
    Int,           // atoi, as the reference reads its numbers: never refused
    Ignored,       // accepted and dropped
    Number,        // parse_number
    Positive,      // parse_positive
    NotNegative,   // parse_not_negative
    Whole,         // parse_whole(lo, hi)
    WholeList,     // parse_whole_list(lo, hi)
    Name,          // one of `names`
    Custom,        // the function `custom`
};

struct Name { const char *name; int value; };
const Name kTimeStepModes[] = {{"reference", MGCFD_DT_REFERENCE}, {"global", MGCFD_DT_GLOBAL}, {"local", MGCFD_DT_LOCAL},
                               {"local-legacy", MGCFD_DT_LOCAL_LEGACY}, {"local_legacy", MGCFD_DT_LOCAL_LEGACY}, {nullptr, 0}};
const Name kCycleShapes[] = {{"V", MGCFD_CYCLE_V}, {"v", MGCFD_CYCLE_V}, {"W", MGCFD_CYCLE_W}, {"w", MGCFD_CYCLE_W}, {"F", MGCFD_CYCLE_F}, {"f", MGCFD_CYCLE_F}, {nullptr, 0}};
const Name kLimiters[] = {{"none", MGCFD_LIMITER_NONE}, {"barth-jespersen", MGCFD_LIMITER_BARTH_JESPERSEN}, {"venkatakrishnan", MGCFD_LIMITER_VENKATAKRISHNAN}, {nullptr, 0}};
const Name kFaceGradients[] = {{"averaged", MGCFD_FACE_GRADIENT_AVERAGED}, {"corrected", MGCFD_FACE_GRADIENT_CORRECTED}, {nullptr, 0}};
const Name kSaLengths[] = {{"wall", MGCFD_SA_LENGTH_WALL}, {"des", MGCFD_SA_LENGTH_DES}, {"ddes", MGCFD_SA_LENGTH_DDES}, {nullptr, 0}};

// the field of Config a value goes to, whatever its type
struct Dest {
    bool Config::*b = nullptr;
    int Config::*i = nullptr;
    double Config::*d = nullptr;
    std::string Config::*s = nullptr;
    std::vector<int> Config::*v = nullptr;
    Dest() {}
    Dest(bool Config::*p) : b(p) {}
    Dest(int Config::*p) : i(p) {}
    Dest(double Config::*p) : d(p) {}
    Dest(std::string Config::*p) : s(p) {}
    Dest(std::vector<int> Config::*p) : v(p) {}
};

// how an option's value is read: a kind, and what that kind needs
struct Reader {
    Read kind;
    int lo, hi;                                  // Whole, WholeList
    const Name *names;                           // Name
    bool (*custom)(Config &, const char *);      // Custom
    Reader(Read k, int l = 0, int h = 0, const Name *n = nullptr, bool (*f)(Config &, const char *) = nullptr) : kind(k), lo(l), hi(h), names(n), custom(f) {}
};
Reader whole(int lo, int hi) { return {Read::Whole, lo, hi}; }
Reader whole_list(int lo, int hi) { return {Read::WholeList, lo, hi}; }
Reader one_of(const Name *names) { return {Read::Name, 0, 0, names}; }
Reader by(bool (*custom)(Config &, const char *)) { return {Read::Custom, 0, 0, nullptr, custom}; }

struct Option {
    const char *cli;                  // --cli on the command line, or none
    char letter;                      // -l, or 0
    const char *key;                  // the key of a config file, or none
    int has_arg;                      // kNoArg; kArg; kOptArg: --cli, --cli=X or --cli X on the command line, Y, X or N in a config file
    Reader read;
    Dest dest = {};
    bool Config::*given = nullptr;    // raised by every accepted value (of a kOptArg option: the option's own switch)
    const char *expected = nullptr;   // "ERROR: ...: expected <this>"; none: the phrase of the kind (expected_phrase)
    bool config_warns = false;        // a config file's bad value is a warning on stdout and the run goes on
};

constexpr int kNoArg = no_argument, kArg = required_argument, kOptArg = optional_argument;
const Option kOptions[] = {
    // the reference's (src/Base/config.cpp:32-47, 81-157)
    {"help", 'h', nullptr, kNoArg, by(help_and_stop)},
    {"config-filepath", 'c', nullptr, kArg, by(set_config_filepath)},
    {"input-file", 'i', "input_file", kArg, Read::String, &Config::input_file},
    {"input-directory", 'd', "input_file_directory", kArg, Read::String, &Config::input_file_directory},
    {"papi_config_file", 'p', "papi_config_file", kArg, Read::String, &Config::papi_config_file},
    {"output-file-prefix", 'o', "output_file_prefix", kArg, Read::String, &Config::output_file_prefix},
    {"mesh-duplicate-count", 'm', "mesh_duplicate_count", kArg, Read::Int, &Config::mesh_duplicate_count},
    {"num-cycles", 'g', "cycles", kArg, Read::Int, &Config::num_cycles},
    {"validate-result", 'v', nullptr, kNoArg, Read::Flag, &Config::validate_result},
    {"output-variables", 0, "output_variables", kNoArg, Read::Flag, &Config::output_variables},
    {"output-fluxes", 0, "output_fluxes", kNoArg, Read::Flag, &Config::output_fluxes},
    {"output-step-factors", 0, "output_step_factors", kNoArg, Read::Flag, &Config::output_step_factors},
    // extensions
    {"device", 0, nullptr, kArg, Read::Int, &Config::device},
    {"no-timers", 0, nullptr, kNoArg, Read::FlagOff, &Config::timers},
    {"no-indirect-rw", 0, nullptr, kNoArg, Read::FlagOff, &Config::indirect_rw},
    {"fast", 0, nullptr, kNoArg, Read::Flag, &Config::fast_math},
    {"legacy-ordering", 0, nullptr, kNoArg, Read::Flag, &Config::legacy_ordering},
    {"gpus", 0, nullptr, kArg, Read::Int, &Config::gpus},
    {"gpus-share-device", 0, nullptr, kNoArg, Read::Flag, &Config::gpus_share_device},
    {"loop-timers", 0, nullptr, kNoArg, Read::Flag, &Config::loop_timers},
    {"gpus-partition", 0, nullptr, kNoArg, Read::Flag, &Config::gpus_partition},
    {"output-loads", 0, nullptr, kNoArg, Read::Flag, &Config::output_loads},
    {"loads-reference", 0, nullptr, kArg, by(set_loads_reference), {}, nullptr, "S,c,x,y,z (five numbers, S and c positive)"},
    {"mach", 0, "ff_mach", kArg, Read::Number, &Config::ff_mach, &Config::free_stream_given, nullptr, true},
    {"alpha", 0, "angle_of_attack", kArg, Read::Number, &Config::angle_of_attack, &Config::free_stream_given, nullptr, true},
    {"polar", 0, nullptr, kArg, by(set_polar), {}, nullptr, "A0:A1:N (two angles in degrees and a count of at least 1)"},
    {"time-step", 0, "time_step", kArg, one_of(kTimeStepModes), &Config::time_step_mode, &Config::time_step_given, "reference, global, local or local-legacy"},
    {"cfl", 0, "cfl", kArg, Read::Positive, &Config::cfl, &Config::time_step_given},
    {"residual-smoothing", 0, "residual_smoothing", kArg, Read::Positive, &Config::smoothing_eps, &Config::smoothing_given},
    {"smoothing-iterations", 0, "smoothing_iterations", kArg, whole(0, MGCFD_MAX_SMOOTHING_ITERATIONS), &Config::smoothing_iterations, &Config::smoothing_iterations_given},
    {"physical-time-step", 0, "physical_time_step", kArg, Read::Positive, &Config::dual_dt, &Config::dual_given},
    {"time-steps", 0, "time_steps", kArg, whole(1, kMaxTimeSteps), &Config::time_steps, &Config::dual_extras_given},
    {"dual-time-clamp", 0, "dual_time_clamp", kArg, Read::Positive, &Config::dual_clamp, &Config::dual_extras_given},
    {"bdf-order", 0, "bdf_order", kArg, whole(1, 2), &Config::bdf_order, &Config::dual_extras_given, "1 or 2"},
    {"jst", 0, "jst", kNoArg, Read::Flag, &Config::jst_given},
    {"fas", 0, "fas", kNoArg, Read::Flag, &Config::fas},
    {"cycle", 0, nullptr, kArg, one_of(kCycleShapes), &Config::cycle_shape, nullptr, "V, W or F"},
    {"pre-sweeps", 0, nullptr, kArg, whole_list(1, MGCFD_MAX_CYCLE_SWEEPS), &Config::pre_sweeps},
    {"post-sweeps", 0, nullptr, kArg, whole_list(0, MGCFD_MAX_CYCLE_SWEEPS), &Config::post_sweeps},
    {"fmg-cycles", 0, nullptr, kArg, whole_list(0, MGCFD_MAX_ADVANCE_CYCLES), &Config::fmg_cycles},
    {"jst-kappa2", 0, "jst_kappa2", kArg, Read::NotNegative, &Config::jst_kappa2, &Config::jst_given},
    {"jst-kappa4", 0, "jst_kappa4", kArg, Read::NotNegative, &Config::jst_kappa4, &Config::jst_given},
    {"jst-levels", 0, "jst_levels", kArg, whole(0, kMaxJstLevels), &Config::jst_levels, &Config::jst_given},
    {"viscosity", 0, "viscosity", kArg, Read::Positive, &Config::viscosity, &Config::viscosity_given},
    {"reynolds", 0, "reynolds", kArg, Read::Positive, &Config::reynolds, &Config::reynolds_given},
    {"ref-length", 0, "ref_length", kArg, Read::Positive, &Config::ref_length, &Config::viscous_extras_given},
    {"prandtl", 0, "prandtl", kArg, Read::Positive, &Config::prandtl, &Config::viscous_extras_given},
    {"viscous-cfl", 0, "viscous_cfl", kArg, by(set_viscous_cfl), {}, nullptr, "a finite number above zero"},
    {"no-slip", 0, "no_slip", kNoArg, by(set_no_slip)},
    {"viscous-levels", 0, "viscous_levels", kArg, whole(0, kMaxJstLevels), &Config::viscous_levels, &Config::viscous_extras_given},
    {"sutherland", 0, "sutherland", kNoArg, Read::Flag, &Config::sutherland},
    {"sutherland-tref", 0, "sutherland_tref", kArg, Read::Positive, &Config::sutherland_tref, &Config::model_extras_given},
    {"sutherland-s", 0, "sutherland_s", kArg, Read::Positive, &Config::sutherland_s, &Config::model_extras_given},
    {"prandtl-turbulent", 0, "prandtl_turbulent", kArg, Read::Positive, &Config::prandtl_turbulent, &Config::model_extras_given},
    {"smagorinsky", 0, "smagorinsky", kOptArg, Read::Positive, &Config::smagorinsky_cs, &Config::smagorinsky, "a finite constant above zero"},
    {"wall-damping", 0, "wall_damping", kOptArg, Read::Positive, &Config::wall_kappa, &Config::wall_damping, "a finite constant above zero"},
    {"spalart-allmaras", 0, "spalart_allmaras", kOptArg, Read::Positive, &Config::sa_ratio, &Config::spalart_allmaras, "a finite ratio above zero"},
    {"loads-friction", 0, nullptr, kNoArg, Read::Flag, &Config::loads_friction},
    {"output-surface", 0, nullptr, kNoArg, Read::Flag, &Config::output_surface},
    {"wall-temperature", 0, "wall_temperature", kArg, by(set_wall_temperature), {}, nullptr, "a finite number above zero"},
    {"wall-temperature-ratio", 0, "wall_temperature_ratio", kArg, by(set_wall_temperature_ratio), {}, nullptr, "a finite number above zero"},
    {"wall-heat-flux", 0, "wall_heat_flux", kArg, by(set_wall_heat_flux), {}, nullptr, "a finite number"},
    {"loads-heat", 0, "loads_heat", kNoArg, Read::Flag, &Config::loads_heat},
    {"face-gradient", 0, "face_gradient", kArg, one_of(kFaceGradients), &Config::face_gradient, &Config::face_gradient_given, "averaged or corrected"},
    {"sa-time-accurate", 0, "sa_time_accurate", kNoArg, by(set_sa_time_accurate)},
    {"sa-length", 0, "sa_length", kArg, one_of(kSaLengths), &Config::sa_length, &Config::sa_unsteady_given, "wall, des or ddes"},
    {"sa-cdes", 0, "sa_cdes", kArg, Read::Positive, &Config::sa_cdes, &Config::sa_unsteady_given},
    {"output-statistics", 0, nullptr, kNoArg, Read::Flag, &Config::output_statistics},
    {"statistics-start", 0, nullptr, kArg, whole(0, kMaxTimeSteps), &Config::statistics_start, &Config::statistics_start_given},
    {"upwind", 0, "upwind", kNoArg, Read::Flag, &Config::upwind_given},
    {"upwind-levels", 0, "upwind_levels", kArg, whole(0, kMaxJstLevels), &Config::upwind_levels, &Config::upwind_given},
    {"muscl-levels", 0, "muscl_levels", kArg, whole(0, kMaxJstLevels), &Config::muscl_levels_said, &Config::upwind_given},
    {"limiter", 0, "limiter", kArg, one_of(kLimiters), &Config::limiter, &Config::upwind_given, "none, barth-jespersen or venkatakrishnan"},
    {"venkat-k", 0, "venkat_k", kArg, Read::Positive, &Config::venkat_k, &Config::upwind_given},
    {"entropy-fix", 0, "entropy_fix", kArg, by(set_entropy_fix), {}, nullptr, "a number 0 ... 1"},
    // keys of a config file alone (src/Base/config.cpp:81-157)
    {nullptr, 0, "config_filepath", kArg, Read::String, &Config::config_filepath},
    {nullptr, 0, "omp_num_threads", kArg, Read::Ignored},      // (no OpenMP here)
    {nullptr, 0, "output_old_variables", kNoArg, Read::Flag, &Config::output_old_variables},
    {nullptr, 0, "output_edge_fluxes", kNoArg, Read::Flag, &Config::output_edge_fluxes},
    {nullptr, 0, "output_volumes", kNoArg, Read::Flag, &Config::output_volumes},
};
constexpr int kFirstOptionCode = 1000;   // getopt_long's code of kOptions[k] is kFirstOptionCode + k: above every short letter

std::string expected_phrase(const Option &o)
{
    if (o.expected) return o.expected;
    switch (o.read.kind) {
        case Read::Number: return "a number";
        case Read::Positive: return "a finite number above zero";
        case Read::NotNegative: return "a finite number, zero or above";
        case Read::Whole: return "a whole number " + std::to_string(o.read.lo) + " ... " + std::to_string(o.read.hi);
        case Read::WholeList: return "whole numbers " + std::to_string(o.read.lo) + " ... " + std::to_string(o.read.hi) + ", comma separated";
        default: return "";
    }
}

// the value of one option into its field; false: refused
bool read_value(const Option &o, Config &c, const char *text)
{
    switch (o.read.kind) {
        case Read::Flag: c.*o.dest.b = true; return true;
        case Read::FlagOff: c.*o.dest.b = false; return true;
        case Read::String: c.*o.dest.s = text; return true;
        case Read::Int: c.*o.dest.i = std::atoi(text); return true;
        case Read::Ignored: return true;
        case Read::Number: return parse_number(text, &(c.*o.dest.d));
        case Read::Positive: return parse_positive(text, &(c.*o.dest.d));
        case Read::NotNegative: return parse_not_negative(text, &(c.*o.dest.d));
        case Read::Whole: return parse_whole(text, o.read.lo, o.read.hi, &(c.*o.dest.i));
        case Read::WholeList: return parse_whole_list(text, o.read.lo, o.read.hi, &(c.*o.dest.v));
        case Read::Name:
            for (const Name *n = o.read.names; n->name; n++)
                if (std::strcmp(text, n->name) == 0) {
                    c.*o.dest.i = n->value;
                    return true;
                }
            return false;
        case Read::Custom: return o.read.custom(c, text);
    }
    return false;
}

// One option with its value (none: a flag, or an optional value left out), from the command line or from a config file.
// A refused value is reported as its source has it: the command line ends the parsing (false); a config file marks the run
// (config_bad) and is read on.
bool apply_option(const Option &o, Config &c, const char *text, bool from_config_file)
{
    if (from_config_file && o.has_arg == no_argument && std::strcmp(text, "Y") != 0) return true;   // (a flag is set by Y alone)
    if (from_config_file && o.has_arg == optional_argument) {
        if (std::strcmp(text, "N") == 0) return true;
        if (std::strcmp(text, "Y") == 0) text = nullptr;
    }
    if ((text || o.has_arg != optional_argument) && !read_value(o, c, text)) {
        const std::string expected = expected_phrase(o);
        if (expected.empty()) return false;
        if (!from_config_file) {
            std::fprintf(stderr, "ERROR: --%s=%s: expected %s\n", o.cli, text, expected.c_str());
            return false;
        }
        if (o.config_warns) std::printf("WARNING: %s = '%s' is not a number.\n", o.key, text);
        else {
            std::fprintf(stderr, "ERROR: %s = '%s': expected %s%s\n", o.key, text, o.has_arg == optional_argument ? "Y or " : "", expected.c_str());
            c.config_bad = true;
        }
        return true;
    }
    if (o.given) c.*o.given = true;
    return true;
}

std::string trim(const std::string &s)
{
    size_t b = s.find_first_not_of(" \t\r\n");
    if (b == std::string::npos) return "";
    return s.substr(b, s.find_last_not_of(" \t\r\n") - b + 1);
}

void set_param(Config &c, const std::string &key, const std::string &value)
{
    for (const Option &o : kOptions)
        if (o.key && key == o.key) {
            apply_option(o, c, value.c_str(), true);
            return;
        }
    std::printf("WARNING: Unknown key '%s' encountered during parsing of config file.\n", key.c_str());
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
    // flag sets exactly its own field.)  getopt_long's tables are made from kOptions.
    std::vector<option> long_opts;
    std::string letters;
    for (const Option &o : kOptions) {
        if (!o.cli) continue;
        long_opts.push_back({o.cli, o.has_arg, nullptr, kFirstOptionCode + int(&o - kOptions)});
        if (o.letter) letters += o.has_arg == required_argument ? std::string{o.letter, ':'} : std::string{o.letter};
    }
    long_opts.push_back({nullptr, 0, nullptr, 0});
    int optc;
    while ((optc = getopt_long(argc, argv, letters.c_str(), long_opts.data(), nullptr)) != -1) {
        const Option *o = nullptr;      // (a long option comes back as its code, a short one as its letter, anything else as '?')
        for (const Option &s : kOptions)
            if (s.cli && (optc == s.letter || optc == kFirstOptionCode + int(&s - kOptions))) o = &s;
        if (!o) {
            std::printf("Unknown command line parameter '%c'\n", optc);
            continue;
        }
        // --smagorinsky, --smagorinsky=CS or --smagorinsky CS (the next word, where it does not start another option)
        const char *arg = optarg;
        if (o->has_arg == optional_argument && !arg && optind < argc && argv[optind][0] != '-') arg = argv[optind++];
        if (!apply_option(*o, c, arg, false)) return false;
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

// the rules between options that main() applies once parse_arguments has let the run pass (so behind a config file's refused value)
bool check_combinations(const Config &c)
{
    if (c.output_loads && c.gpus > 1 && !c.gpus_partition) {
        std::fprintf(stderr, "ERROR: --output-loads runs on one GPU only, or on --gpus N with --gpus-partition (every level split over the ranks)\n");
        return false;
    }
    if (c.smoothing_given && c.smoothing_iterations > 0 && c.gpus > 1 && c.gpus_partition) {
        std::fprintf(stderr, "ERROR: residual smoothing (--residual-smoothing) does not run with --gpus-partition: a level split over GPUs would need a halo exchange per Jacobi iteration\n");
        return false;
    }
    if (c.jst_given && c.jst_levels > 0 && c.gpus > 1 && c.gpus_partition) {
        std::fprintf(stderr, "ERROR: the JST dissipation (--jst) does not run with --gpus-partition: a level split over GPUs would need its sensor and Laplacian exchanged per stage\n");
        return false;
    }
    if (c.viscous() && c.viscous_levels > 0 && c.gpus > 1 && c.gpus_partition) {
        std::fprintf(stderr, "ERROR: the viscous terms (--viscosity, --reynolds) do not run with --gpus-partition: a level split over GPUs would need its node stresses exchanged per stage\n");
        return false;
    }
    if (c.dual_given && c.gpus > 1 && c.gpus_partition) {
        std::fprintf(stderr, "ERROR: dual time stepping (--physical-time-step) does not run with --gpus-partition: levels split over GPUs are out of scope\n");
        return false;
    }
    if (c.fas && c.gpus > 1) {
        std::fprintf(stderr, "ERROR: FAS multigrid (--fas) runs on one GPU only: levels split over GPUs, or one level per GPU, would need the residuals, the forcing and the corrections exchanged\n");
        return false;
    }
    if ((c.cycle_given() || !c.fmg_cycles.empty()) && c.gpus > 1) {
        std::fprintf(stderr, "ERROR: --cycle, --pre-sweeps, --post-sweeps and --fmg-cycles run on one GPU only: levels split over GPUs, or one level per GPU, run the default cycle\n");
        return false;
    }
    if (!c.fmg_cycles.empty() && (c.dual_given || c.polar)) {
        std::fprintf(stderr, "ERROR: a full-multigrid start (--fmg-cycles) does not run with --physical-time-step or --polar\n");
        return false;
    }
    if (c.dual_given && c.polar) {
        std::fprintf(stderr, "ERROR: dual time stepping (--physical-time-step) does not run with --polar\n");
        return false;
    }
    if (c.polar && c.gpus > 1 && !c.gpus_partition) {
        std::fprintf(stderr, "ERROR: --polar runs on one GPU only, or on --gpus N with --gpus-partition (every level split over the ranks)\n");
        return false;
    }
    return true;
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
    if (!check_combinations(conf)) return 1;
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
