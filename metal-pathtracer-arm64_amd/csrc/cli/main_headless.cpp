// PathTracerHeadless — command-line front end of the MI355X backend.
// Flag set, defaults, override order (scene file first, CLI second), default output naming and the final
// report line follow the reference's src/main_headless.mm:26-606.  Backends: `hip` (default; `metal` is
// accepted as an alias so existing command lines keep working).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <filesystem>
#include <iomanip>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "headless.h"
#include "image_writer.h"
#include "scene_manager.h"

namespace fs = std::filesystem;

namespace {

struct CliOptions {
    std::string scene;
    bool sceneProvided = false;
    std::string assetDir;
    std::string outputPath;
    uint32_t width = 0, height = 0;
    bool widthSet = false, heightSet = false;
    uint32_t sppTotal = 1024;
    uint32_t maxDepth = 0;
    bool maxDepthSet = false;
    uint32_t threads = 0;
    uint32_t seed = 0;
    bool seedSet = false;
    float envRotationDegrees = 0.0f;
    bool envRotationSet = false;
    float envIntensity = 0.0f;
    bool envIntensitySet = false;
    uint32_t tonemapMode = 0;
    bool tonemapSet = false;
    float exposure = 0.0f;
    bool exposureSet = false;
    bool enableSoftwareRayTracing = false, enableSoftwareRayTracingSet = false;
    bool enableMnee = false, enableMneeSet = false;
    uint32_t metalSemantics = 0;
    uint32_t devices = 1;            // --devices: GPUs of this node the frame is spread over (0 = all visible)
    std::string aovExrPath;          // --aovExr: also write the first-hit feature layers
    bool denoise = false;            // --denoise: filter the frame, guided by the first-hit feature buffers (include/ptr_post.h)
    uint32_t denoiseIterations = 0;  // --denoiseIterations: a-trous passes (0 = the filter's default)
    bool denoiseSampleVariance = false;   // --denoiseVariance=sample: the filter's variance from the per-pixel sample covariance (include/ptr_stats.h)
    bool adaptive = false;           // --adaptive: the frame in rounds over the pixels whose error is above a threshold (include/ptr_adaptive.h)
    float adaptiveThreshold = 0.0f;  // --adaptive=<threshold>
    bool adaptiveThresholdSet = false;
    uint32_t adaptiveMinSpp = 0, adaptiveStep = 0;   // --adaptiveMinSpp / --adaptiveStep (0 = the default)
    std::vector<uint32_t> snapshots; // --snapshots: also write the image at these samples per pixel on the way to --sppTotal (include/ptr_frame.h)
    uint32_t backendSemantics = 0;   // what --backend / --enableEmbree imply; an explicit --semantics overrides it
    bool semanticsSet = false;
    std::string formatString = "exr";
    ptr::ImageFileFormat format = ptr::ImageFileFormat::EXR;
    bool rgbaExr = false;
    bool verbose = false;
};

// PTR_METAL_MEDIA | PTR_METAL_THIN | PTR_METAL_FACE_NORMAL | PTR_METAL_SPECULAR | PTR_METAL_SSS | PTR_METAL_PBR | PTR_METAL_CLAMPS
constexpr uint32_t kMetalSemanticsAll = 127u;
// ... and PTR_METAL_ENV_LOD, the prefiltered environment lookups (--semantics=metal-envlod)
constexpr uint32_t kMetalSemanticsEnvLod = kMetalSemanticsAll | 128u;
// ... and PTR_METAL_RAY_DIFF, the first-hit ray differentials of textured lookups (--semantics=metal-raydiff / metal-envlod-raydiff)
constexpr uint32_t kMetalSemanticsRayDiff = kMetalSemanticsAll | 256u;
constexpr uint32_t kMetalSemanticsEnvLodRayDiff = kMetalSemanticsEnvLod | 256u;

void printUsage(const char* exe) {
    std::cout << "Usage: " << exe << " [options]\n\n"
              << "Required:\n"
              << "  --scene=<path>                Path to a .scene file\n\n"
              << "Rendering overrides:\n"
              << "  --width=<int>                 Override render width (>=8)\n"
              << "  --height=<int>                Override render height (>=8)\n"
              << "  --sppTotal=<int>              Total samples to accumulate (default 1024)\n"
              << "  --maxDepth=<int>              Override max path depth\n"
              << "  --threads=<int>               Accepted for compatibility (CPU backends only)\n"
              << "  --seed=<int>                  Fixed RNG seed (0 = default stream)\n"
              << "  --enableSoftwareRayTracing[=0|1]  Accepted; this backend always traces in software\n"
              << "  --enableMnee[=0|1]             Enable MNEE caustics (default 0)\n\n"
              << "Environment overrides:\n"
              << "  --envRotation=<deg>           Environment rotation in degrees\n"
              << "  --envIntensity=<float>        Environment intensity multiplier\n\n"
              << "Backend selection:\n"
              << "  --backend=<hip|embree|metal>   hip / embree: Embree-parity integrator (default); metal: as --semantics=metal\n"
              << "  --enableEmbree[=0|1]           Same as --backend=embree (1) / --backend=metal (0)\n"
              << "  --semantics=<embree|metal|metal-envlod|metal-raydiff|metal-envlod-raydiff>\n"
              << "                                 Integrator semantics: embree = parity with the reference's Embree backend\n"
              << "                                 (default); metal = plus the Metal kernel's absorbing media, thin-walled glass, ray-facing\n"
              << "                                 glass normals, rough-metal VNDF formulas, subsurface scattering (scene: renderer sss=...),\n"
              << "                                 three-lobe PBR with transmission, the Metal kernel's clamp variants; metal-envlod = metal\n"
              << "                                 plus environment lookups at a mip level chosen by roughness after glossy bounces and\n"
              << "                                 for environment samples of glossy materials; metal-raydiff = metal plus anisotropic\n"
              << "                                 texture lookups from camera-ray differentials at the first hit of textured meshes;\n"
              << "                                 metal-envlod-raydiff = both\n"
              << "  --devices=<int>                GPUs of this node to spread the frame over (default 1, 0 = all visible)\n"
              << "  --assets=<dir>                 Directory for relative mesh/env paths\n\n"
              << "Tonemapping overrides (for LDR outputs):\n"
              << "  --tonemap=<1|2|3|4>           1=Linear, 2=ACES, 3=Reinhard, 4=Hable\n"
              << "  --exposure=<float>            Exposure in stops\n\n"
              << "Output controls:\n"
              << "  --output=<path>               Output filename\n"
              << "  --format=<exr|pfm|ppm>        Output format (default exr)\n"
              << "  --rgbaExr[=0|1]               Write RGBA EXR with colorspace attribute (Embree-backend layout)\n"
              << "  --aovExr=<path>               Also write beauty + first-hit albedo / normal / depth layers (denoiser inputs) as one EXR\n"
              << "  --denoise[=0|1]               Denoise the image (and the beauty layer of --aovExr) with the edge-avoiding a-trous\n"
              << "                                wavelet filter guided by the first-hit albedo / normal / depth (default 0)\n"
              << "  --denoiseIterations=<1..8>    A-trous passes of --denoise (default 5)\n"
              << "  --denoiseVariance=<spatial|sample>  Variance of --denoise's luminance edge-stop: spatial = estimated from a 7x7 window of\n"
              << "                                the image (default); sample = measured per pixel from the frame's own samples (needs\n"
              << "                                --denoise, --sppTotal >= 2 and --devices=1)\n"
              << "  --adaptive[=<threshold>]      Render in rounds: every pixel gets --adaptiveMinSpp samples, then only the pixels whose\n"
              << "                                relative standard error (or a neighbour's) is above the threshold go on, up to\n"
              << "                                --sppTotal samples (default threshold 0.05; needs --devices=1)\n"
              << "  --adaptiveMinSpp=<n>          Samples of the first round of --adaptive (>= 2, default 8)\n"
              << "  --adaptiveStep=<n>            Samples of every later round of --adaptive (>= 1, default 8)\n"
              << "  --snapshots=<n1,n2,...>       Also write the image at n1, n2, ... samples per pixel on the way to --sppTotal, next to\n"
              << "                                --output as <stem>.<n><ext> (strictly ascending, each >= 2 and below --sppTotal; the frame\n"
              << "                                is continued, not rendered again; snapshots are not denoised; needs --devices=1, not\n"
              << "                                with --adaptive)\n"
              << "  --verbose                     Print progress\n"
              << "  --help                        Show this message\n";
}

bool parseBoolFlag(const std::string& value, bool defaultIfEmpty, bool& out) {
    if (value.empty()) {
        out = defaultIfEmpty;
        return true;
    }
    std::string l;
    for (char c : value) l.push_back(static_cast<char>(std::tolower(static_cast<unsigned char>(c))));
    if (l == "1" || l == "true" || l == "yes") {
        out = true;
        return true;
    }
    if (l == "0" || l == "false" || l == "no") {
        out = false;
        return true;
    }
    return false;
}

bool parseOptions(int argc, const char** argv, CliOptions& o, std::string& error) {
    for (int i = 1; i < argc; ++i) {
        std::string arg = argv[i], value;
        const size_t eq = arg.find('=');
        const bool inlineValue = eq != std::string::npos;
        if (inlineValue) {
            value = arg.substr(eq + 1);
            arg = arg.substr(0, eq);
        }
        auto need = [&](const char* name) {
            if (inlineValue) return true;
            if (i + 1 >= argc) {
                error = std::string(name) + " requires a value";
                return false;
            }
            value = argv[++i];
            return true;
        };
        auto intArg = [&](const char* name, int minValue, uint32_t& dst, bool* setFlag) {
            if (!need(name)) return false;
            try {
                const int parsed = std::stoi(value);
                if (parsed < minValue) {
                    error = std::string(name) + " must be >= " + std::to_string(minValue);
                    return false;
                }
                dst = static_cast<uint32_t>(parsed);
                if (setFlag) *setFlag = true;
                return true;
            } catch (...) {
                error = std::string("Invalid integer for ") + name;
                return false;
            }
        };
        auto floatArg = [&](const char* name, float& dst, bool& setFlag) {
            if (!need(name)) return false;
            try {
                dst = std::stof(value);
                setFlag = true;
                return true;
            } catch (...) {
                error = std::string("Invalid float for ") + name;
                return false;
            }
        };
        auto boolArg = [&](const char* name, bool& dst, bool* setFlag) {
            bool flag = true;
            if (!parseBoolFlag(inlineValue ? value : std::string(), true, flag)) {
                error = std::string("Invalid value for ") + name;
                return false;
            }
            dst = flag;
            if (setFlag) *setFlag = true;
            return true;
        };

        if (arg == "--help" || arg == "-h") {
            printUsage(argv[0]);
            std::exit(0);
        } else if (arg == "--verbose" || arg == "-v") {
            if (!boolArg("--verbose", o.verbose, nullptr)) return false;
        } else if (arg == "--scene") {
            if (!need("--scene")) return false;
            o.scene = value;
            o.sceneProvided = true;
        } else if (arg == "--assets") {
            if (!need("--assets")) return false;
            o.assetDir = value;
        } else if (arg == "--output") {
            if (!need("--output")) return false;
            o.outputPath = value;
        } else if (arg == "--width") {
            if (!intArg("--width", 8, o.width, &o.widthSet)) return false;
        } else if (arg == "--height") {
            if (!intArg("--height", 8, o.height, &o.heightSet)) return false;
        } else if (arg == "--sppTotal") {
            if (!intArg("--sppTotal", 1, o.sppTotal, nullptr)) return false;
        } else if (arg == "--maxDepth") {
            if (!intArg("--maxDepth", 1, o.maxDepth, &o.maxDepthSet)) return false;
        } else if (arg == "--threads") {
            if (!intArg("--threads", 1, o.threads, nullptr)) return false;
        } else if (arg == "--seed") {
            if (!need("--seed")) return false;
            try {
                o.seed = static_cast<uint32_t>(std::stoul(value));
                o.seedSet = true;
            } catch (...) {
                error = "Invalid integer for --seed";
                return false;
            }
        } else if (arg == "--envRotation") {
            if (!floatArg("--envRotation", o.envRotationDegrees, o.envRotationSet)) return false;
        } else if (arg == "--envIntensity") {
            if (!floatArg("--envIntensity", o.envIntensity, o.envIntensitySet)) return false;
            o.envIntensity = std::max(o.envIntensity, 0.0f);
        } else if (arg == "--tonemap") {
            if (!intArg("--tonemap", 1, o.tonemapMode, &o.tonemapSet)) return false;
            if (o.tonemapMode > 4) {
                error = "--tonemap must be in [1,4]";
                return false;
            }
        } else if (arg == "--exposure") {
            if (!floatArg("--exposure", o.exposure, o.exposureSet)) return false;
        } else if (arg == "--enableSoftwareRayTracing") {
            if (!boolArg("--enableSoftwareRayTracing", o.enableSoftwareRayTracing, &o.enableSoftwareRayTracingSet)) return false;
        } else if (arg == "--enableMnee") {
            if (!boolArg("--enableMnee", o.enableMnee, &o.enableMneeSet)) return false;
        } else if (arg == "--rgbaExr") {
            if (!boolArg("--rgbaExr", o.rgbaExr, nullptr)) return false;
        } else if (arg == "--format") {
            if (!need("--format")) return false;
            o.formatString = value;
        } else if (arg == "--devices") {
            if (!intArg("--devices", 0, o.devices, nullptr)) return false;
        } else if (arg == "--aovExr") {
            if (!need("--aovExr")) return false;
            o.aovExrPath = value;
        } else if (arg == "--denoise") {
            if (!boolArg("--denoise", o.denoise, nullptr)) return false;
        } else if (arg == "--denoiseIterations") {
            if (!intArg("--denoiseIterations", 1, o.denoiseIterations, nullptr)) return false;
            if (o.denoiseIterations > PTR_DENOISE_MAX_ITERATIONS) {
                error = "--denoiseIterations must be in [1,8]";
                return false;
            }
        } else if (arg == "--denoiseVariance") {
            if (!need("--denoiseVariance")) return false;
            if (value != "spatial" && value != "sample") {
                error = "Invalid value for --denoiseVariance (expected spatial or sample)";
                return false;
            }
            o.denoiseSampleVariance = value == "sample";
        } else if (arg == "--adaptive") {
            o.adaptive = true;
            if (inlineValue) {
                size_t used = 0;
                try {
                    o.adaptiveThreshold = std::stof(value, &used);
                } catch (...) {
                    used = 0;
                }
                if (used == 0 || used != value.size() || !std::isfinite(o.adaptiveThreshold) || o.adaptiveThreshold < 0.0f) {
                    error = "Invalid value for --adaptive (expected a finite threshold >= 0)";
                    return false;
                }
                o.adaptiveThresholdSet = true;
            }
        } else if (arg == "--adaptiveMinSpp") {
            if (!intArg("--adaptiveMinSpp", 2, o.adaptiveMinSpp, nullptr)) return false;
        } else if (arg == "--adaptiveStep") {
            if (!intArg("--adaptiveStep", 1, o.adaptiveStep, nullptr)) return false;
        } else if (arg == "--snapshots") {
            if (!need("--snapshots")) return false;
            o.snapshots.clear();
            for (size_t at = 0; at <= value.size();) {
                const size_t comma = std::min(value.find(',', at), value.size());
                const std::string item = value.substr(at, comma - at);
                size_t used = 0;
                unsigned long n = 0;
                try {
                    n = std::stoul(item, &used);
                } catch (...) {
                    used = 0;
                }
                if (item.empty() || used != item.size() || item[0] == '-' || n > 0xFFFFFFFFul) {
                    error = "Invalid value for --snapshots (expected a comma-separated list of sample counts)";
                    return false;
                }
                o.snapshots.push_back(static_cast<uint32_t>(n));
                at = comma + 1;
            }
        } else if (arg == "--semantics") {
            if (!need("--semantics")) return false;
            if (value == "metal") {
                o.metalSemantics = kMetalSemanticsAll;
            } else if (value == "metal-envlod") {
                o.metalSemantics = kMetalSemanticsEnvLod;
            } else if (value == "metal-raydiff") {
                o.metalSemantics = kMetalSemanticsRayDiff;
            } else if (value == "metal-envlod-raydiff") {
                o.metalSemantics = kMetalSemanticsEnvLodRayDiff;
            } else if (value == "embree") {
                o.metalSemantics = 0u;
            } else {
                error = "Invalid value for --semantics (expected embree, metal, metal-envlod, metal-raydiff or metal-envlod-raydiff)";
                return false;
            }
            o.semanticsSet = true;
        } else if (arg == "--backend") {
            // The reference picks between its two renderers here (main_headless.mm:344-362).  This build has one device
            // path; what the reference's backends differ in is the integrator, so the names select its semantics:
            // embree -> the Embree-parity integrator, metal -> the Metal kernel's.  An explicit --semantics wins.
            if (!need("--backend")) return false;
            std::string l;
            for (char c : value) l.push_back(static_cast<char>(std::tolower(static_cast<unsigned char>(c))));
            if (l == "metal") {
                o.backendSemantics = kMetalSemanticsAll;
            } else if (l == "embree" || l == "hip") {
                o.backendSemantics = 0u;
            } else {
                error = "Invalid value for --backend (expected hip, embree or metal)";
                return false;
            }
        } else if (arg == "--enableEmbree") {
            // main_headless.mm:363-371: --enableEmbree[=1] = --backend=embree, --enableEmbree=0 = --backend=metal
            bool flag = true;
            if (!boolArg("--enableEmbree", flag, nullptr)) return false;
            o.backendSemantics = flag ? 0u : kMetalSemanticsAll;
        } else {
            error = "Unknown option: " + arg;
            return false;
        }
    }
    if (!o.semanticsSet) o.metalSemantics = o.backendSemantics;
    if (!o.sceneProvided) {
        error = "--scene is required";
        return false;
    }
    if (o.denoiseSampleVariance && !o.denoise) {
        error = "--denoiseVariance=sample requires --denoise";
        return false;
    }
    if (o.denoiseSampleVariance && o.sppTotal < 2u) {
        error = "--denoiseVariance=sample requires --sppTotal >= 2";
        return false;
    }
    if ((o.adaptiveMinSpp || o.adaptiveStep) && !o.adaptive) {
        error = "--adaptiveMinSpp and --adaptiveStep require --adaptive";
        return false;
    }
    if (o.adaptive && o.sppTotal < (o.adaptiveMinSpp ? o.adaptiveMinSpp : 8u)) {
        error = "--adaptive requires --sppTotal (the most samples a pixel gets) >= --adaptiveMinSpp";
        return false;
    }
    for (size_t i = 0; i < o.snapshots.size(); ++i) {
        if (o.snapshots[i] < 2u || o.snapshots[i] >= o.sppTotal || (i > 0 && o.snapshots[i] <= o.snapshots[i - 1])) {
            error = "--snapshots must be strictly ascending, each >= 2 and below --sppTotal";
            return false;
        }
    }
    if (!ptr::ParseImageFileFormat(o.formatString, o.format)) {
        error = "Unknown format: " + o.formatString;
        return false;
    }
    return true;
}

// The combinations of modes that parse but do not render: reported without the usage text, before the scene is loaded.  Empty = none.
std::string modeRefusal(const CliOptions& o) {
    const std::string devices = "; it cannot be combined with --devices=" + std::to_string(o.devices);
    if (o.denoiseSampleVariance && o.devices != 1u) return "--denoiseVariance=sample renders on one device" + devices;
    if (o.adaptive && o.devices != 1u) return "--adaptive renders on one device" + devices;
    if (!o.snapshots.empty() && o.adaptive) return "--snapshots continues a uniform frame; it cannot be combined with --adaptive";
    if (!o.snapshots.empty() && o.devices != 1u) return "--snapshots renders on one device" + devices;
    return std::string();
}

std::string sanitizeSceneName(const std::string& input) {
    if (input.empty()) return "scene";
    std::string name = fs::path(input).stem().string();
    if (name.empty()) name = input;
    for (char& c : name) {
        if (!(std::isalnum(static_cast<unsigned char>(c)) || c == '-' || c == '_')) c = '_';
    }
    return name;
}

}  // namespace

int main(int argc, const char** argv) {
    CliOptions options;
    std::string error;
    if (!parseOptions(argc, argv, options, error)) {
        if (!error.empty()) std::cerr << "Error: " << error << "\n\n";
        printUsage(argv[0]);
        return 1;
    }

    const std::string refusal = modeRefusal(options);
    if (!refusal.empty()) {
        std::cerr << "Error: " << refusal << std::endl;
        return 1;
    }

    ptr::SceneManager sceneManager(options.assetDir);
    ptr::SceneResources resources;
    ptr::RenderSettings settings{};
    std::string sceneError;
    // a value that looks like a path (or names an existing file) is loaded directly; anything else is a scene
    // identifier looked up in the scene directory (main_headless.mm:389-396, 486-506)
    bool sceneIsPath;
    {
        const std::filesystem::path scenePath(options.scene);
        std::error_code ec;
        sceneIsPath = scenePath.extension() == ".scene" || scenePath.has_parent_path() || scenePath.is_absolute() ||
                      std::filesystem::exists(scenePath, ec);
    }
    const bool sceneLoaded = sceneIsPath ? sceneManager.loadSceneFromPath(options.scene, resources, settings, &sceneError)
                                         : sceneManager.loadScene(options.scene, resources, settings, &sceneError);
    if (!sceneLoaded) {
        std::cerr << "Failed to load scene: " << options.scene << std::endl;
        if (!sceneError.empty()) std::cerr << sceneError << std::endl;
        if (!sceneManager.scenes().empty()) {
            std::cerr << "Available scenes:" << std::endl;
            for (const auto& info : sceneManager.scenes()) std::cerr << "  " << info.identifier << std::endl;
        }
        return 1;
    }

    // CLI overrides apply after the scene file (main_headless.mm:418-449)
    if (options.widthSet) settings.renderWidth = options.width;
    if (options.heightSet) settings.renderHeight = options.height;
    if (options.maxDepthSet) settings.maxDepth = options.maxDepth;
    if (options.seedSet) settings.fixedRngSeed = options.seed;
    if (options.tonemapSet) settings.tonemapMode = options.tonemapMode;
    if (options.exposureSet) settings.exposure = options.exposure;
    if (options.envRotationSet) settings.environmentRotation = options.envRotationDegrees * static_cast<float>(3.14159265358979323846 / 180.0);
    if (options.envIntensitySet) settings.environmentIntensity = std::max(options.envIntensity, 0.0f);
    if (options.enableSoftwareRayTracingSet) settings.enableSoftwareRayTracing = options.enableSoftwareRayTracing;
    if (options.enableMneeSet) settings.enableMnee = options.enableMnee;
    settings.metalSemantics = options.metalSemantics;
    if (settings.renderWidth == 0) settings.renderWidth = 1280u;
    if (settings.renderHeight == 0) settings.renderHeight = 720u;

    ptr::HeadlessScene scene{};
    scene.source = options.scene;
    scene.isPath = sceneIsPath;
    scene.resources = &resources;
    ptr::HeadlessCamera camera{};
    camera.target = settings.cameraTarget;
    camera.distance = settings.cameraDistance;
    camera.yaw = settings.cameraYaw;
    camera.pitch = settings.cameraPitch;
    camera.verticalFov = settings.cameraVerticalFov;
    camera.defocusAngle = settings.cameraDefocusAngle;
    camera.focusDistance = settings.cameraFocusDistance;

    auto hipRenderer = std::make_unique<ptr::HipHeadlessRenderer>();
    hipRenderer->setDeviceCount(static_cast<int>(options.devices));
    hipRenderer->setCaptureAovs(!options.aovExrPath.empty());
    if (options.denoise) {
        PtrDenoiseParams denoiseParams;
        ptr_denoise_default_params(&denoiseParams);
        if (options.denoiseIterations) denoiseParams.iterations = options.denoiseIterations;
        hipRenderer->setDenoise(&denoiseParams);
        hipRenderer->setDenoiseVariance(options.denoiseSampleVariance);
    }
    if (options.adaptive) {
        PtrAdaptiveParams adaptiveParams;
        ptr_adaptive_default_params(&adaptiveParams, options.sppTotal);
        if (options.adaptiveThresholdSet) adaptiveParams.threshold = options.adaptiveThreshold;
        if (options.adaptiveMinSpp) adaptiveParams.minSpp = options.adaptiveMinSpp;
        if (options.adaptiveStep) adaptiveParams.stepSpp = options.adaptiveStep;
        hipRenderer->setAdaptive(&adaptiveParams);
    }
    // where the image goes (the default name carries the size), and how a linear image is written there
    auto outputPathFor = [&](uint32_t width, uint32_t height) {
        if (!options.outputPath.empty()) return options.outputPath;
        std::ostringstream name;
        name << sanitizeSceneName(options.scene) << "_" << width << "x" << height << "." << ptr::FormatExtension(options.format);
        return (fs::path("renders") / name.str()).string();
    };
    auto makeParentDirectory = [](const fs::path& path) {
        std::error_code ec;
        if (!path.parent_path().empty()) fs::create_directories(path.parent_path(), ec);
    };
    auto writeImageFile = [&](const fs::path& path, const float* linearRGB, uint32_t width, uint32_t height, std::string& writeError) {
        makeParentDirectory(path);
        if (options.format == ptr::ImageFileFormat::EXR && options.rgbaExr) {
            std::vector<float> rgba(static_cast<size_t>(width) * height * 4u, 1.0f);
            for (size_t i = 0; i < static_cast<size_t>(width) * height; ++i) {
                rgba[i * 4 + 0] = linearRGB[i * 3 + 0];
                rgba[i * 4 + 1] = linearRGB[i * 3 + 1];
                rgba[i * 4 + 2] = linearRGB[i * 3 + 2];
            }
            return ptr::WriteExrRgba(path.string(), rgba.data(), width, height, "Linear sRGB", &writeError);
        }
        ptr::TonemapSettings tm;
        tm.tonemapMode = settings.tonemapMode;
        tm.acesVariant = settings.acesVariant;
        tm.exposure = settings.exposure;
        tm.reinhardWhitePoint = settings.reinhardWhitePoint;
        return ptr::WriteImage(path.string(), options.format, linearRGB, width, height, tm, &writeError);
    };
    if (!options.snapshots.empty()) {
        // <stem>.<n><ext> next to the output, in its format and with its tonemap options
        hipRenderer->setSnapshots(options.snapshots, [&](uint32_t spp, uint32_t width, uint32_t height, const float* linearRGB, std::string& sinkError) {
            const fs::path out(outputPathFor(width, height));
            const fs::path path = out.parent_path() / (out.stem().string() + "." + std::to_string(spp) + out.extension().string());
            if (!writeImageFile(path, linearRGB, width, height, sinkError)) {
                sinkError = "failed to write snapshot " + path.string() + ": " + sinkError;
                return false;
            }
            std::cout << "Snapshot at " << spp << " spp written to: " << path << std::endl;
            return true;
        });
    }
    const ptr::HipHeadlessRenderer* const hip = hipRenderer.get();
    std::unique_ptr<ptr::IHeadlessRenderer> renderer = std::move(hipRenderer);
    ptr::HeadlessRenderOutput output;
    std::string renderError;
    if (!renderer->render(scene, camera, settings, options.sppTotal, options.verbose, output, renderError)) {
        std::cerr << "Render failed: " << renderError << std::endl;
        return 1;
    }

    const std::string outputPath = outputPathFor(output.width, output.height);
    const fs::path outFs(outputPath);
    std::string writeError;
    const bool ok = writeImageFile(outFs, output.linearRGB.data(), output.width, output.height, writeError);
    if (!ok) {
        std::cerr << "Failed to write output image: " << writeError << std::endl;
        return 1;
    }
    if (!options.aovExrPath.empty()) {
        const fs::path aovFs(options.aovExrPath);
        makeParentDirectory(aovFs);
        if (!ptr::WriteExrAovs(options.aovExrPath, output.linearRGB.data(), hip->aovAlbedo().data(), hip->aovNormal().data(), output.width,
                               output.height, &writeError)) {
            std::cerr << "Failed to write AOV image: " << writeError << std::endl;
            return 1;
        }
        std::cout << "Feature layers written to: " << aovFs << std::endl;
    }

    if (options.adaptive) {
        const double meanSpp = static_cast<double>(hip->lastAdaptiveInfo().totalSamples) / (static_cast<double>(output.width) * output.height);
        std::cout << "Rendered up to " << output.samples << " spp (" << std::fixed << std::setprecision(2) << meanSpp << " spp on average, "
                  << hip->lastAdaptiveInfo().rounds << " rounds) at " << output.width << "x" << output.height << " in " << output.totalSeconds << " s"
                  << " (~" << std::setprecision(3) << output.avgMsPerSample << " ms/sample)." << std::endl;
    } else {
        std::cout << "Rendered " << output.samples << " spp at " << output.width << "x" << output.height << " in "
                  << std::fixed << std::setprecision(2) << output.totalSeconds << " s"
                  << " (~" << std::setprecision(3) << output.avgMsPerSample << " ms/sample)." << std::endl;
    }
    std::cout << "Output written to: " << outFs << std::endl;
    return 0;
}
