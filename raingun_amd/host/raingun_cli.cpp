// raingun_cli.cpp — the `raingun` binary (src/main.rs:98-132 + src/render.rs)
// on the native host layer (libraingun_host.so: YAML scene, textures, PNG) and
// the HIP renderer (libraingun_hip.so: rg_render_image).
//
//   raingun [-w PIXELS] [-h PIXELS] [--4k|--hd] [--draft] [--samples N] [--adaptive T]
//           [--eye X,Y,Z] [--look-at X,Y,Z] [--up X,Y,Z] [--aperture R --focus D] [--light-radius R[,R...]]
//           [--aov LAYERS] [--ao K[,RADIUS[,BIAS]]] [--ambient R,G,B] [--ao-filter R[,NMIN]] [-o FILE] [--gpu N] FILE
//
// --ambient R,G,B (or one number for grey; not in the reference, which has no ambient light): `out.png` becomes
// the frame of rg_render_image_ambient -- the --samples frame plus this radiance from every open direction, weighted
// by the filtered AO pass.  It needs --ao, refuses --adaptive, and combines with --samples, the camera, the lens and
// --light-radius.  A colour that is negative or not finite is an argument error.
// --ao-filter R[,NMIN] (R 0..8, NMIN in [0, 1], default 0.9): the edge-stopping filter of the AO pass
// (rg_ao_filter).  It needs --ao.  With --ambient the default is 2,0.9 and `--ao-filter 0` composes the raw pass;
// given explicitly, `out.ao.png` shows the filtered pass (without the flag it stays the raw one).
// --ao K[,RADIUS[,BIAS]] (not in the reference): next to `-o out.png` the run also writes `out.ao.png`, the
// ambient occlusion of the frame (rg_render_ao): K x K rays (K 1..8) over the hemisphere above each pixel's
// primary hit, occluded by hits within RADIUS (> 0, `inf` the default), leaving BIAS (>= 0, default 1e-13)
// above the surface; grey, the byte the Rust `(ao * 255.0) as u8`, alpha 255 (raingun_amd/ao.py visualize).
// It honours the size flags and the camera, is independent of --samples, --aperture and --light-radius, and
// runs after the beauty frame, outside its timing line.  A malformed value is an argument error.  Without
// --ao nothing changes.
// --aov LAYERS (not in the reference): a comma list of body, depth, normal, uv, albedo, or `all`.  Next to
// `-o out.png` the run also writes `out.<layer>.png` for each named layer: what lies under each pixel
// (rg_render_aov), as the pictures raingun_amd/aov.py states in numpy (visualize): every cast the Rust
// `f32 as u8`, alpha 255.  It honours the size flags and the camera; --samples and --adaptive affect only
// the beauty frame.  An unknown layer name is an argument error.  Without --aov nothing changes.
// --eye / --look-at / --up (not in the reference, whose view is from the origin down -z): the camera
// (rg_camera_look_at, rg_scene_set_camera).  --up defaults to 0,1,0; --eye without --look-at looks down
// -z from the eye; a malformed triple or a rejected look-at is an argument error.  No camera key in the YAML.
// --aperture R --focus D (not in the reference): a thin lens of radius R (world units) focused on the plane D
// forward lengths away (rg_scene_set_lens): depth of field from the N x N rays of --samples.  They go
// together, need --samples 2 or more and refuse --adaptive (argument errors otherwise), and combine with
// the camera and the size flags.
// --light-radius R (not in the reference): every spherical light of the scene gets the radius R in world units
// (rg_scene_set_light_radii): soft shadows from the N x N rays of --samples.  A comma list gives one radius per
// light in YAML order (0 for a directional light).  It needs --samples 2 or more and refuses --adaptive
// (argument errors otherwise), and combines with the camera and the lens.
// --adaptive T (0..256; not in the reference): the N x N rays only for pixels whose 8-neighbourhood
// contrast in the 1-sample frame is at least T (rg_render_image_aa_adaptive); accepted with
// --samples 1, where it has no effect.
// --samples N (1..8, default 1; not in the reference): N x N rays per pixel on the
// regular sub-pixel grid, box-filtered (rg_render_image_aa); --draft leaves it alone.
// Flag semantics follow construct_app / RenderOptions::from (main.rs:21-96,
// clap 2.23 overrides_with: the last of --4k/--hd wins; --draft forces
// 800x600 and caps the recursion depth at 4, main.rs:74-75, 119-123, and
// overrides --4k/--hd/--width/--height, main.rs:47-54).  Panic sites of the
// reference (`expect(...)`) print the same message and exit with status 101,
// Rust's panic status; argument errors exit with 1 like clap.  `--preview`
// (piston window) has no display on an MI355X node: it renders without one.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/raingun.h"
#include "../../include/raingun_host.h"

namespace {

const char *kUsage =
    "USAGE:\n    raingun [FLAGS] [OPTIONS] <FILE>\n";

const char *kHelp =
    "raingun 0.1.0\n"
    "Magnus Bergmark <magnus.bergmark@gmail.com>\n\n"
    "USAGE:\n    raingun [FLAGS] [OPTIONS] <FILE>\n\n"
    "FLAGS:\n"
    "        --4k         Renders in 4K resolution. Explicit width/height overrides.\n"
    "        --draft      Renders in 800x600 and lower quality settings.\n"
    "        --hd         Renders in 1080 (HD) resolution. Explicit width/height overrides.\n"
    "        --help       Prints help information\n"
    "        --preview    Shows render progress in a window (not available: renders without one).\n"
    "    -V, --version    Prints version information\n\n"
    "OPTIONS:\n"
    "        --eye <X,Y,Z>          Camera position (default 0,0,0).\n"
    "        --look-at <X,Y,Z>      Point the camera looks at (default: straight down -z from the eye).\n"
    "        --up <X,Y,Z>           Up hint of --look-at (default 0,1,0).\n"
    "        --aperture <R>         Lens radius in world units (with --focus and --samples 2 or more).\n"
    "        --focus <D>            Distance of the plane in focus, in lengths of the forward vector.\n"
    "        --light-radius <R>     Radius of every spherical light in world units, or R,R,.. one per light (with --samples 2 or more).\n"
    "        --ambient <R,G,B>      Ambient light of this colour (or one number), weighted by the filtered --ao pass, added to the frame.\n"
    "        --ao-filter <R[,NMIN]> Edge-stopping filter of the --ao pass: radius 0..8 (0: off), least normal cosine (default 0.9); with --ambient the default is 2,0.9.\n"
    "        --ao <K[,RADIUS[,BIAS]]>  Also write FILENAME.ao.png: ambient occlusion, K x K rays per pixel (1..8), hits within RADIUS occlude (default inf).\n"
    "        --aov <LAYERS>         Also write FILENAME.<layer>.png for each of body,depth,normal,uv,albedo (or all).\n"
    "        --adaptive <T>         Adaptive anti-aliasing: the N x N rays only where the 1-sample frame's contrast is at least T (0..256).\n"
    "        --gpu <N>              HIP device to render on (default 0).\n"
    "    -h, --height <PIXELS>      Height of output image.\n"
    "    -o, --output <FILENAME>    Specify filename of the rendered image.\n"
    "        --samples <N>          Anti-aliasing: N x N rays per pixel, box-filtered (1..8, default 1).\n"
    "    -w, --width <PIXELS>       Width of output image.\n\n"
    "ARGS:\n"
    "    <FILE>    The scene definition file, in YAML format.\n";

[[noreturn]] void clap_error(const std::string &msg) {
    std::fprintf(stderr, "error: %s\n\n%s\nFor more information try --help\n", msg.c_str(), kUsage);
    std::exit(1);
}

[[noreturn]] void panic(const std::string &msg) {
    std::fflush(stdout);
    std::fprintf(stderr, "thread 'main' panicked at '%s', src/main.rs\n", msg.c_str());
    std::exit(101);
}

struct Args {
    bool draft = false, hd = false, uhd = false, preview = false;
    const char *width = nullptr, *height = nullptr, *output = nullptr, *input = nullptr, *samples = nullptr,
               *adaptive = nullptr, *eye = nullptr, *look_at = nullptr, *up = nullptr, *aov = nullptr, *ao = nullptr, *ambient = nullptr, *ao_filter = nullptr, *aperture = nullptr, *focus = nullptr,
               *light_radius = nullptr;
    int gpu = 0;
};

struct RenderOptions {  // render.rs:32-46
    uint32_t width = 800, height = 600;
    uint32_t samples = 1;  // N x N rays per pixel (--samples)
    bool has_adaptive = false;
    uint32_t adaptive = 0;  // contrast threshold (--adaptive)
    bool has_depth = false;
    uint32_t max_recursion_depth = 0;
    bool has_camera = false;  // --eye / --look-at / --up
    rg_camera camera{};
    bool has_lens = false;  // --aperture / --focus
    rg_lens lens{0.0, 1.0};
    std::vector<double> light_radii;  // --light-radius as given: one number, or one per light (empty: no flag)
    bool aov[5] = {false, false, false, false, false};  // --aov: body, depth, normal, uv, albedo
    bool any_aov = false;
    bool has_ao = false;  // --ao
    rg_ao ao{1, 0, INFINITY, 1e-13};
    bool has_ambient = false;  // --ambient
    float ambient[3] = {0.0f, 0.0f, 0.0f};
    bool has_filter = false;  // --ao-filter given explicitly
    rg_ao_filter_desc filter{0, 0.9f};  // radius 0: no filter (with --ambient and no --ao-filter: 2, 0.9)
};

const char *const kLayers[5] = {"body", "depth", "normal", "uv", "albedo"};

bool parse_triple(const char *s, double out[3]) {  // "X,Y,Z": three finite numbers, nothing else
    if (!s) return false;
    for (int k = 0; k < 3; ++k) {
        if (!*s || *s == ' ' || *s == '\t') return false;  // (strtod would skip the blank)
        char *end = nullptr;
        out[k] = std::strtod(s, &end);
        if (end == s || !(out[k] - out[k] == 0.0)) return false;
        if (*end != (k < 2 ? ',' : '\0')) return false;
        s = end + 1;
    }
    return true;
}

bool parse_f64(const char *s, double *out) {  // one finite number, nothing else
    if (!s || !*s || *s == ' ' || *s == '\t') return false;
    char *end = nullptr;
    *out = std::strtod(s, &end);
    return end != s && *end == '\0' && *out - *out == 0.0;
}

bool parse_u32(const char *s, uint32_t *out) {  // str::parse::<u32>
    if (!s || !*s) return false;
    const char *p = s;
    if (*p == '+') ++p;
    if (!*p) return false;
    uint64_t v = 0;
    for (; *p; ++p) {
        if (*p < '0' || *p > '9') return false;
        v = v * 10 + (uint64_t)(*p - '0');
        if (v > 0xFFFFFFFFull) return false;
    }
    *out = (uint32_t)v;
    return true;
}

Args parse_args(int argc, char **argv) {
    Args a;
    bool only_positional = false;
    auto take_value = [&](int &i, const std::string &name, const char *inline_value) -> const char * {
        if (inline_value) return inline_value;
        if (i + 1 >= argc) clap_error("The argument '" + name + "' requires a value but none was supplied");
        return argv[++i];
    };
    for (int i = 1; i < argc; ++i) {
        const char *arg = argv[i];
        if (only_positional || arg[0] != '-' || !arg[1]) {
            if (a.input) clap_error(std::string("Found argument '") + arg + "' which wasn't expected, or isn't valid in this context");
            a.input = arg;
            continue;
        }
        if (!std::strcmp(arg, "--")) { only_positional = true; continue; }
        if (arg[1] == '-') {
            std::string name(arg + 2);
            const char *val = nullptr;
            size_t eq = name.find('=');
            if (eq != std::string::npos) { val = arg + 2 + eq + 1; name = name.substr(0, eq); }
            if (name == "width") a.width = take_value(i, "--width <PIXELS>", val);
            else if (name == "height") a.height = take_value(i, "--height <PIXELS>", val);
            else if (name == "output") a.output = take_value(i, "--output <FILENAME>", val);
            else if (name == "gpu") a.gpu = std::atoi(take_value(i, "--gpu <N>", val));
            else if (name == "samples") a.samples = take_value(i, "--samples <N>", val);
            else if (name == "adaptive") a.adaptive = take_value(i, "--adaptive <T>", val);
            else if (name == "eye") a.eye = take_value(i, "--eye <X,Y,Z>", val);
            else if (name == "look-at") a.look_at = take_value(i, "--look-at <X,Y,Z>", val);
            else if (name == "up") a.up = take_value(i, "--up <X,Y,Z>", val);
            else if (name == "ao") a.ao = take_value(i, "--ao <K[,RADIUS[,BIAS]]>", val);
            else if (name == "ambient") a.ambient = take_value(i, "--ambient <R,G,B>", val);
            else if (name == "ao-filter") a.ao_filter = take_value(i, "--ao-filter <R[,NMIN]>", val);
            else if (name == "aov") a.aov = take_value(i, "--aov <LAYERS>", val);
            else if (name == "aperture") a.aperture = take_value(i, "--aperture <R>", val);
            else if (name == "focus") a.focus = take_value(i, "--focus <D>", val);
            else if (name == "light-radius") a.light_radius = take_value(i, "--light-radius <R>", val);
            else if (val) clap_error("Found argument '" + std::string(arg) + "' which wasn't expected, or isn't valid in this context");
            else if (name == "4k") { a.uhd = true; a.hd = false; }   // overrides_with("hd")
            else if (name == "hd") { a.hd = true; a.uhd = false; }   // overrides_with("4k")
            else if (name == "draft") a.draft = true;
            else if (name == "preview") a.preview = true;
            else if (name == "help") { std::fputs(kHelp, stdout); std::exit(0); }
            else if (name == "version") { std::puts("raingun 0.1.0"); std::exit(0); }
            else clap_error("Found argument '" + std::string(arg) + "' which wasn't expected, or isn't valid in this context");
            continue;
        }
        const char c = arg[1];
        const char *inl = arg[2] ? arg + 2 : nullptr;
        if (inl && *inl == '=') ++inl;
        if (c == 'w') a.width = take_value(i, "--width <PIXELS>", inl);
        else if (c == 'h') a.height = take_value(i, "--height <PIXELS>", inl);
        else if (c == 'o') a.output = take_value(i, "--output <FILENAME>", inl);
        else if (c == 'V' && !inl) { std::puts("raingun 0.1.0"); std::exit(0); }
        else clap_error("Found argument '" + std::string(arg) + "' which wasn't expected, or isn't valid in this context");
    }
    if (!a.input) clap_error("The following required arguments were not provided:\n    <FILE>");
    return a;
}

RenderOptions options_from(const Args &a) {  // main.rs:70-96
    RenderOptions o;
    if (a.samples) {
        if (!parse_u32(a.samples, &o.samples)) panic("Could not parse samples: ParseIntError { kind: InvalidDigit }");
        if (o.samples < 1 || o.samples > 8)
            clap_error(std::string("Invalid value for '--samples <N>': ") + a.samples + " is not between 1 and 8");
    }
    if (a.adaptive) {
        if (!parse_u32(a.adaptive, &o.adaptive)) panic("Could not parse adaptive: ParseIntError { kind: InvalidDigit }");
        if (o.adaptive > 256)
            clap_error(std::string("Invalid value for '--adaptive <T>': ") + a.adaptive + " is not between 0 and 256");
        o.has_adaptive = true;
    }
    if (a.aov) {
        const std::string spec = a.aov;
        for (size_t pos = 0; spec != "all";) {
            const size_t comma = spec.find(',', pos);
            const std::string name = spec.substr(pos, comma == std::string::npos ? std::string::npos : comma - pos);
            int k = 0;
            while (k < 5 && name != kLayers[k]) ++k;
            if (k == 5) clap_error(std::string("Invalid value for '--aov <LAYERS>': ") + a.aov);
            o.aov[k] = true;
            if (comma == std::string::npos) break;
            pos = comma + 1;
        }
        for (int k = 0; k < 5; ++k) o.any_aov |= (o.aov[k] |= spec == "all");
    }
    if (a.ao) {  // K[,RADIUS[,BIAS]]: K 1..8; RADIUS > 0, inf allowed; BIAS finite, >= 0
        const std::string spec = a.ao;
        std::vector<std::string> parts;
        for (size_t pos = 0;;) {
            const size_t comma = spec.find(',', pos);
            parts.push_back(spec.substr(pos, comma == std::string::npos ? std::string::npos : comma - pos));
            if (comma == std::string::npos) break;
            pos = comma + 1;
        }
        auto number = [](const std::string &t, double *out) {  // one number (inf allowed), nothing else
            if (t.empty() || t[0] == ' ' || t[0] == '\t') return false;
            char *end = nullptr;
            *out = std::strtod(t.c_str(), &end);
            return end != t.c_str() && *end == '\0';
        };
        bool good = parts.size() >= 1 && parts.size() <= 3 && parse_u32(parts[0].c_str(), &o.ao.samples) &&
                    o.ao.samples >= 1 && o.ao.samples <= 8;
        if (good && parts.size() > 1) good = number(parts[1], &o.ao.radius) && o.ao.radius > 0.0;
        if (good && parts.size() > 2) good = number(parts[2], &o.ao.bias) && o.ao.bias - o.ao.bias == 0.0 && o.ao.bias >= 0.0;
        if (!good) clap_error(std::string("Invalid value for '--ao <K[,RADIUS[,BIAS]]>': ") + a.ao);
        o.has_ao = true;
    }
    auto split = [](const std::string &spec) {
        std::vector<std::string> parts;
        for (size_t pos = 0;;) {
            const size_t comma = spec.find(',', pos);
            parts.push_back(spec.substr(pos, comma == std::string::npos ? std::string::npos : comma - pos));
            if (comma == std::string::npos) break;
            pos = comma + 1;
        }
        return parts;
    };
    // a number of --ambient / --ao-filter: decimal digits, '.', an exponent and signs only (no hex floats, no inf or
    // nan: what raingun_amd/ambient.py accepts), and within f32's range
    auto decimal = [](const std::string &t, double *out) {
        if (t.empty() || t.find_first_not_of("0123456789.eE+-") != std::string::npos) return false;
        return parse_f64(t.c_str(), out) && std::fabs(*out) <= 3.4028234663852886e38;
    };
    if (a.ambient) {  // R,G,B or one number: finite, >= 0 as f32
        const std::vector<std::string> parts = split(a.ambient);
        bool good = parts.size() == 1 || parts.size() == 3;
        for (size_t k = 0; good && k < parts.size(); ++k) {
            double v = 0.0;
            good = decimal(parts[k], &v);
            const float f = good ? (float)v : 0.0f;
            good = good && f >= 0.0f;
            if (parts.size() == 1) o.ambient[0] = o.ambient[1] = o.ambient[2] = f;
            else o.ambient[k] = f;
        }
        if (!good) clap_error(std::string("Invalid value for '--ambient <R,G,B>': ") + a.ambient);
        if (!o.has_ao) clap_error("The argument '--ambient <R,G,B>' needs '--ao <K[,RADIUS[,BIAS]]>'");
        if (o.has_adaptive) clap_error("The argument '--ambient <R,G,B>' cannot be used with '--adaptive <T>'");
        o.has_ambient = true;
        o.filter.radius = 2;
    }
    if (a.ao_filter) {  // R[,NMIN]: R 0..8; NMIN in [0, 1] as f32
        const std::vector<std::string> parts = split(a.ao_filter);
        double nmin = 0.9;
        bool good = parts.size() >= 1 && parts.size() <= 2 && parse_u32(parts[0].c_str(), &o.filter.radius) && o.filter.radius <= 8;
        if (good && parts.size() > 1) good = decimal(parts[1], &nmin);
        o.filter.normal_min = good ? (float)nmin : 0.0f;
        good = good && o.filter.normal_min >= 0.0f && o.filter.normal_min <= 1.0f;
        if (!good) clap_error(std::string("Invalid value for '--ao-filter <R[,NMIN]>': ") + a.ao_filter);
        if (!o.has_ao) clap_error("The argument '--ao-filter <R[,NMIN]>' needs '--ao <K[,RADIUS[,BIAS]]>'");
        o.has_filter = true;
    }
    if (a.up && !a.look_at) clap_error("The argument '--up <X,Y,Z>' needs '--look-at <X,Y,Z>'");
    if (a.eye || a.look_at) {
        double eye[3] = {0.0, 0.0, 0.0}, target[3], up[3] = {0.0, 1.0, 0.0};
        if (a.eye && !parse_triple(a.eye, eye)) clap_error(std::string("Invalid value for '--eye <X,Y,Z>': ") + a.eye);
        if (a.look_at && !parse_triple(a.look_at, target))
            clap_error(std::string("Invalid value for '--look-at <X,Y,Z>': ") + a.look_at);
        if (a.up && !parse_triple(a.up, up)) clap_error(std::string("Invalid value for '--up <X,Y,Z>': ") + a.up);
        if (a.look_at) {
            if (rg_camera_look_at(eye, target, up, &o.camera) != RG_OK)
                clap_error("Invalid camera: --look-at equals --eye, or --up is parallel to the view direction");
        } else {  // straight down -z from the eye
            const rg_camera c = {{eye[0], eye[1], eye[2]}, {1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, -1.0}};
            o.camera = c;
        }
        o.has_camera = true;
    }
    if (a.aperture || a.focus) {
        if (!a.aperture || !a.focus) clap_error("The arguments '--aperture <R>' and '--focus <D>' go together");
        if (!parse_f64(a.aperture, &o.lens.aperture) || o.lens.aperture < 0.0)
            clap_error(std::string("Invalid value for '--aperture <R>': ") + a.aperture);
        if (!parse_f64(a.focus, &o.lens.focus) || !(o.lens.focus > 0.0))
            clap_error(std::string("Invalid value for '--focus <D>': ") + a.focus);
        if (o.samples < 2) clap_error("The argument '--aperture <R>' needs '--samples <N>' of 2 or more");
        if (o.has_adaptive) clap_error("The argument '--aperture <R>' cannot be used with '--adaptive <T>'");
        o.has_lens = true;
    }
    if (a.light_radius) {
        const std::string spec = a.light_radius;
        for (size_t pos = 0;;) {
            const size_t comma = spec.find(',', pos);
            const std::string item = spec.substr(pos, comma == std::string::npos ? std::string::npos : comma - pos);
            double r = 0.0;
            if (!parse_f64(item.c_str(), &r) || r < 0.0)
                clap_error(std::string("Invalid value for '--light-radius <R>': ") + a.light_radius);
            o.light_radii.push_back(r);
            if (comma == std::string::npos) break;
            pos = comma + 1;
        }
        if (o.samples < 2) clap_error("The argument '--light-radius <R>' needs '--samples <N>' of 2 or more");
        if (o.has_adaptive) clap_error("The argument '--light-radius <R>' cannot be used with '--adaptive <T>'");
    }
    if (a.draft) {
        o.has_depth = true;
        o.max_recursion_depth = 4;
        return o;  // --draft overrides width/height (main.rs:47-54)
    }
    if (a.hd) { o.width = 1920; o.height = 1080; }
    else if (a.uhd) { o.width = 3840; o.height = 2160; }
    if (a.width && !parse_u32(a.width, &o.width)) panic("Could not parse width: ParseIntError { kind: InvalidDigit }");
    if (a.height && !parse_u32(a.height, &o.height)) panic("Could not parse height: ParseIntError { kind: InvalidDigit }");
    return o;
}

std::string format_duration(long long ms) {  // render.rs:229-244
    const long long one_minute = 1000 * 60;
    char buf[64];
    if (ms <= 800) std::snprintf(buf, sizeof buf, "%lldms", ms);
    else if (ms <= one_minute) std::snprintf(buf, sizeof buf, "%.2fs", (double)((float)ms / 1000.0f));
    else {
        long long minutes = ms / one_minute;
        std::snprintf(buf, sizeof buf, "%lldm %.2fs", minutes, (double)((float)(ms - minutes * one_minute) / 1000.0f));
    }
    return buf;
}

// PathBuf::set_extension("png"): false when there is no file name.
bool with_png_extension(const std::string &in, std::string &out) {
    std::string path = in;
    while (path.size() > 1 && path.back() == '/') path.pop_back();
    size_t slash = path.rfind('/');
    std::string dir = slash == std::string::npos ? "" : path.substr(0, slash + 1);
    std::string name = slash == std::string::npos ? path : path.substr(slash + 1);
    if (name.empty() || name == "." || name == ".." || path == "/") return false;
    size_t dot = name.rfind('.');
    std::string stem = (dot == std::string::npos || dot == 0) ? name : name.substr(0, dot);
    out = dir + stem + ".png";
    return true;
}

// Path::with_suffix(".<layer>.png") of the output file: out.png -> out.body.png
std::string with_layer_extension(const std::string &path, const char *layer) {
    const size_t slash = path.rfind('/');
    const size_t name0 = slash == std::string::npos ? 0 : slash + 1;
    const size_t dot = path.rfind('.');
    const std::string stem = (dot == std::string::npos || dot <= name0) ? path : path.substr(0, dot);
    return stem + "." + layer + ".png";
}

// Rust `f32 as u8`: truncate, saturate, NaN -> 0.
uint8_t f32_to_u8(float v) {
    if (!(v > 0.0f)) return 0;
    if (v >= 255.0f) return 255;
    return (uint8_t)v;
}

// The picture of layer k (raingun_amd/aov.py visualize): n pixels -> RGBA8.
void visualize(int k, size_t n, const int32_t *body, const double *depth, const float *f, uint8_t *px) {
    double tmin = 0.0, tmax = 0.0;
    bool any = false;
    if (k == 1)
        for (size_t i = 0; i < n; ++i)
            if (std::isfinite(depth[i])) {
                tmin = any ? std::fmin(tmin, depth[i]) : depth[i];
                tmax = any ? std::fmax(tmax, depth[i]) : depth[i];
                any = true;
            }
    for (size_t i = 0; i < n; ++i) {
        uint8_t *p = px + 4 * i;
        p[0] = p[1] = p[2] = 0;
        p[3] = 255;
        if (k == 0) {
            if (body[i] < 0) continue;
            const uint32_t h = (uint32_t)(body[i] + 1) * 2654435761u;
            p[0] = (uint8_t)(h >> 24);
            p[1] = (uint8_t)(h >> 16);
            p[2] = (uint8_t)(h >> 8);
        } else if (k == 1) {
            if (!std::isfinite(depth[i])) continue;
            const double v = tmax == tmin ? 1.0 : 1.0 - (depth[i] - tmin) / (tmax - tmin);
            const float g = (float)v;
            p[0] = p[1] = p[2] = f32_to_u8(g * 255.0f);
        } else if (k == 2) {
            const float *c = f + 3 * i;
            if (c[0] == 0.0f && c[1] == 0.0f && c[2] == 0.0f) continue;
            for (int j = 0; j < 3; ++j) {
                const float half = c[j] * 0.5f;
                const float shifted = half + 0.5f;
                p[j] = f32_to_u8(shifted * 255.0f);
            }
        } else if (k == 3) {
            for (int j = 0; j < 2; ++j) {
                const float frac = f[2 * i + j] - std::floor(f[2 * i + j]);
                p[j] = f32_to_u8(frac * 255.0f);
            }
        } else {
            for (int j = 0; j < 3; ++j) p[j] = f32_to_u8(f[3 * i + j] * 255.0f);  // color.rs:32-37
        }
    }
}

}  // namespace

int main(int argc, char **argv) {
    const Args args = parse_args(argc, argv);
    const RenderOptions opts = options_from(args);
    const std::string input = args.input;
    std::string output;
    if (args.output) {
        output = args.output;
    } else if (!with_png_extension(input, output)) {
        std::printf("Could not guess output filename from %s\n", input.c_str());
        return 2;
    }
    if (args.preview)
        std::fprintf(stderr, "--preview is not supported on this build (no display); rendering without preview\n");

    rgh_scene *loaded = nullptr;
    int32_t st = rgh_scene_load_file(input.c_str(), nullptr, &loaded);  // textures relative to the CWD
    if (st == RGH_ERR_IO) panic(rgh_last_error());
    if (st != RGH_OK) panic(rgh_last_error());
    if (opts.has_depth) rgh_scene_clamp_depth(loaded, opts.max_recursion_depth);  // main.rs:119-123

    rg_scene *scene = nullptr;
    st = rg_scene_create(rgh_scene_desc(loaded), args.gpu, &scene);
    if (st != RG_OK) panic(std::string("rg_scene_create: ") + rg_status_string(st));
    if (opts.has_camera && (st = rg_scene_set_camera(scene, &opts.camera)) != RG_OK)
        panic(std::string("rg_scene_set_camera: ") + rg_status_string(st));
    if (opts.has_lens && (st = rg_scene_set_lens(scene, &opts.lens)) != RG_OK)
        panic(std::string("rg_scene_set_lens: ") + rg_status_string(st));
    if (!opts.light_radii.empty()) {
        // one number: every spherical light (a directional one stays hard); a list: one per light in YAML order
        const rg_scene_desc *desc = rgh_scene_desc(loaded);
        std::vector<double> radii(opts.light_radii);
        if (radii.size() == 1) {
            radii.assign(desc->n_lights, 0.0);
            for (uint32_t l = 0; l < desc->n_lights; ++l)
                if (desc->lights[l].kind == RG_LIGHT_SPHERICAL) radii[l] = opts.light_radii[0];
        } else if (radii.size() != desc->n_lights) {
            clap_error("The argument '--light-radius <R>' lists " + std::to_string(radii.size()) + " radii, the scene has " +
                       std::to_string(desc->n_lights) + " lights");
        }
        if ((st = rg_scene_set_light_radii(scene, radii.data(), (uint32_t)radii.size())) != RG_OK)
            panic(std::string("rg_scene_set_light_radii: ") + rg_status_string(st));
    }
    std::vector<uint8_t> rgba((size_t)opts.width * opts.height * 4);

    std::vector<float> occlusion;  // --ambient: the pass it composed (filtered, or raw at --ao-filter 0)
    rg_ambient term{};
    if (opts.has_ambient) {
        for (int c = 0; c < 3; ++c) term.color[c] = opts.ambient[c];
        term.samples = opts.samples;
        term.ao = opts.ao;
        term.filter_radius = opts.filter.radius;
        term.normal_min = opts.filter.normal_min;
        occlusion.resize((size_t)opts.width * opts.height);
    }
    auto t0 = std::chrono::steady_clock::now();  // render.rs:54-56
    st = opts.has_ambient
             ? rg_render_image_ambient(scene, opts.width, opts.height, &term, rgba.data(), nullptr, occlusion.data(), nullptr)
         : opts.samples > 1 && opts.has_adaptive
             ? rg_render_image_aa_adaptive(scene, opts.width, opts.height, opts.samples, opts.adaptive, rgba.data(), nullptr,
                                           nullptr, nullptr)
         : opts.samples > 1 ? rg_render_image_aa(scene, opts.width, opts.height, opts.samples, rgba.data(), nullptr, nullptr)
                          : rg_render_image(scene, opts.width, opts.height, rgba.data(), nullptr);
    auto t1 = std::chrono::steady_clock::now();
    if (st != RG_OK) panic(rg_status_string(st));
    st = rgh_png_write(output.c_str(), rgba.data(), opts.width, opts.height);  // render.rs:58
    auto t2 = std::chrono::steady_clock::now();
    if (st != RGH_OK) panic(rgh_last_error());
    if (opts.any_aov) {  // after the beauty frame and outside its timing line
        const size_t n = (size_t)opts.width * opts.height;
        std::vector<int32_t> body(opts.aov[0] ? n : 0);
        std::vector<double> depth(opts.aov[1] ? n : 0);
        std::vector<float> normal(opts.aov[2] ? 3 * n : 0), uv(opts.aov[3] ? 2 * n : 0), albedo(opts.aov[4] ? 3 * n : 0);
        const rg_aov layers = {opts.aov[0] ? body.data() : nullptr, opts.aov[1] ? depth.data() : nullptr,
                               opts.aov[2] ? normal.data() : nullptr, opts.aov[3] ? uv.data() : nullptr,
                               opts.aov[4] ? albedo.data() : nullptr};
        st = rg_render_aov(scene, opts.width, opts.height, &layers, nullptr);
        if (st != RG_OK) panic(rg_status_string(st));
        const float *planes[5] = {nullptr, nullptr, normal.data(), uv.data(), albedo.data()};
        for (int k = 0; k < 5; ++k) {
            if (!opts.aov[k]) continue;
            visualize(k, n, body.data(), depth.data(), planes[k], rgba.data());
            st = rgh_png_write(with_layer_extension(output, kLayers[k]).c_str(), rgba.data(), opts.width, opts.height);
            if (st != RGH_OK) panic(rgh_last_error());
        }
    }
    if (opts.has_ao) {  // after the beauty frame and outside its timing line
        const size_t n = (size_t)opts.width * opts.height;
        if (!(opts.has_ambient && opts.has_filter)) {  // the raw pass; else the pass --ambient composed
            occlusion.resize(n);
            st = rg_render_ao(scene, opts.width, opts.height, &opts.ao, occlusion.data(), nullptr);
            if (st != RG_OK) panic(rg_status_string(st));
        }
        if (!opts.has_ambient && opts.has_filter && opts.filter.radius > 0) {  // --ao-filter alone: the filtered pass
            std::vector<int32_t> body(n);
            std::vector<float> normal(3 * n), raw(occlusion);
            const rg_aov guides = {body.data(), nullptr, normal.data(), nullptr, nullptr};
            st = rg_render_aov(scene, opts.width, opts.height, &guides, nullptr);
            if (st == RG_OK)
                st = rg_ao_filter(args.gpu, raw.data(), body.data(), normal.data(), opts.width, opts.height, &opts.filter,
                                  occlusion.data());
            if (st != RG_OK) panic(rg_status_string(st));
        }
        for (size_t i = 0; i < n; ++i) {  // raingun_amd/ao.py visualize
            uint8_t *p = rgba.data() + 4 * i;
            p[0] = p[1] = p[2] = f32_to_u8(occlusion[i] * 255.0f);
            p[3] = 255;
        }
        st = rgh_png_write(with_layer_extension(output, "ao").c_str(), rgba.data(), opts.width, opts.height);
        if (st != RGH_OK) panic(rgh_last_error());
    }
    rg_scene_destroy(scene);
    rgh_scene_free(loaded);

    auto ms = [](std::chrono::steady_clock::duration d) {
        return (long long)std::chrono::duration_cast<std::chrono::milliseconds>(d).count();
    };
    std::printf("%s\t\xe2\x86\x92\t%s\t(%s render, %s write)\n", input.c_str(), output.c_str(),
                format_duration(ms(t1 - t0)).c_str(), format_duration(ms(t2 - t1)).c_str());
    return 0;
}
