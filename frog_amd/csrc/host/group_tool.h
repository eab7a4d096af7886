// group_tool.h -- what the tools over a registered group (AverageImage, FuseLabels) share: leaving on an error, the header
// peek, the positional arguments, a list file's lines, a fused map's type, one inverted chain per image from <transformsDir>/<i>.json, the first output lines, the
// resliced volume an add hands back and its file, the phase timers and the lines that close the run.  Each tool keeps its own
// flags, validation and outputs.  AverageVolumes takes `die` from here.
#ifndef FROG_GROUP_TOOL_H
#define FROG_GROUP_TOOL_H

#include "tool_common.h"

#include <sys/stat.h>
#include <cerrno>
#include <zlib.h>

#include <chrono>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <initializer_list>
#include <iostream>
#include <string>
#include <vector>

// reader threads may still be inflating: leave without running static destructors under them
[[noreturn]] inline void die(const std::string &what)
{
    std::cout << "Error : " << what << std::endl;
    std::_Exit(1);
}

using clk = std::chrono::steady_clock;
inline double seconds(clk::time_point since) { return std::chrono::duration<double>(clk::now() - since).count(); }

// The header of a volume, without inflating its data: `ok` it parses (NIfTI-1: sizeof_hdr == 348; MetaImage: DimSize present,
// frog_volume_geometry), `is_float` it declares a float type (NIfTI-1: datatype 16 FLOAT32 or 64 FLOAT64 at byte 70;
// MetaImage: ElementType, read up to ElementDataFile).
struct VolumeHeader {
    bool ok = false, is_float = false;
};

inline VolumeHeader peek_header(const std::string &path)
{
    auto has_suffix = [&](const char *s) { const size_t n = std::strlen(s); return path.size() >= n && path.compare(path.size() - n, n, s) == 0; };
    VolumeHeader h;
    if (has_suffix(".mhd") || has_suffix(".mha")) {
        uint32_t d[3]; double sp[3], o[3];
        if (frog_volume_geometry(path.c_str(), d, sp, o) != FROG_OK) return h;
        h.ok = true;
        std::ifstream f(path);
        for (std::string line; std::getline(f, line) && line.compare(0, 15, "ElementDataFile") != 0;)
            if (line.compare(0, 11, "ElementType") == 0 && (line.find("MET_FLOAT") != std::string::npos || line.find("MET_DOUBLE") != std::string::npos))
                h.is_float = true;
        return h;
    }
    if (!has_suffix(".nii") && !has_suffix(".nii.gz")) return h;
    gzFile f = gzopen(path.c_str(), "rb");
    if (!f) return h;
    unsigned char bytes[72];
    const bool read = gzread(f, bytes, sizeof bytes) == (int)sizeof bytes;
    gzclose(f);
    int32_t n = 0;
    int16_t datatype = 0;
    std::memcpy(&n, bytes, sizeof n);
    std::memcpy(&datatype, bytes + 70, sizeof datatype);
    h.ok = read && n == 348;
    h.is_float = h.ok && (datatype == 16 || datatype == 64);
    return h;
}

// argv[first], ... up to the first of `flags` go to `positional`; the index of that flag, argc without one.  From there on
// the tool reads its own "flag value" pairs.
inline int positional_arguments(int argc, char *argv[], int first, std::initializer_list<const char *> flags, std::vector<std::string> &positional)
{
    auto is_flag = [&](const char *a) {
        for (const char *f : flags) if (std::strcmp(a, f) == 0) return true;
        return false;
    };
    int a = first;
    for (; a < argc && !is_flag(argv[a]); a++) positional.push_back(argv[a]);
    return a;
}

// the lines of a list file (FROG.py -m's format: one path per line), without their line ends; blank lines are dropped
inline bool read_list(const std::string &path, std::vector<std::string> &lines)
{
    std::ifstream f(path);
    if (!f) return false;
    for (std::string line; std::getline(f, line);) {
        while (!line.empty() && (line.back() == '\r' || line.back() == ' ' || line.back() == '\t')) line.pop_back();
        if (!line.empty()) lines.push_back(line);
    }
    return true;
}

// The type of a fused label map: the first of u8, u16, i16, i32, u32 that holds every one of the ascending `values`; -1 if none
// does.
inline int fused_type(const std::vector<int64_t> &values)
{
    int64_t lo = 0, hi = 0;
    if (!values.empty()) { lo = values.front(); hi = values.back(); }
    const struct { int dtype; int64_t lo, hi; } types[] = {
        { FROG_V_U8, 0, 255 }, { FROG_V_U16, 0, 65535 }, { FROG_V_I16, -32768, 32767 },
        { FROG_V_I32, -2147483647LL - 1, 2147483647LL }, { FROG_V_U32, 0, 4294967295LL } };
    for (const auto &t : types) if (t.lo <= lo && hi <= t.hi) return t.dtype;
    return -1;
}

// <transformsDir>/<i>.json of each of n images, read (`transforms` owns the files from here on) and inverted: every image
// has a chain of its own
inline std::vector<std::vector<frog_chain_link>> inverse_transforms(ChainArguments &transforms, const std::string &transformsDir, size_t n)
{
    std::vector<std::vector<frog_chain_link>> inverse(n);
    for (size_t i = 0; i < n; i++) {
        const std::string path = transformsDir + "/" + std::to_string(i) + ".json";
        frog_transform_file *f = transforms.read(path.c_str());
        if (!f) die("cannot read transform " + path);
        const uint32_t nl = frog_transform_num_links(f);
        inverse[i].resize(nl);
        if (frog_chain_invert_links(frog_transform_links(f), nl, inverse[i].data())) die(path + ": " + frog_last_error());
    }
    return inverse;
}

inline std::vector<frog_chain *> create_chains(const std::vector<std::vector<frog_chain_link>> &inverse, int device)
{
    std::vector<frog_chain *> chains(inverse.size(), nullptr);
    for (size_t i = 0; i < inverse.size(); i++)
        if (frog_chain_create(inverse[i].data(), (uint32_t)inverse[i].size(), device, &chains[i])) die("transform " + std::to_string(i) + ": " + frog_last_error());
    return chains;
}

// The first things a tool leaves behind, once every input is checked: the output directory and the line about the group
// ("images", "label maps") and its grid.
inline void begin_output(const std::string &outDir, size_t n, const char *noun, const frog_volume &grid)
{
    if (mkdir(outDir.c_str(), 0755) != 0 && errno != EEXIST) die("cannot create " + outDir);
    std::cout << n << " " << noun << ", grid " << grid.dims[0] << " x " << grid.dims[1] << " x " << grid.dims[2] << " (spacing " << grid.spacing[0]
              << ", origin " << grid.origin[0] << " " << grid.origin[1] << " " << grid.origin[2] << ")" << std::endl;
}

// -wt 1: the resliced volume of image i, which the add fills, and its file <outDir>/<stem><i>.nii.gz
struct ReslicedVolume {
    frog_volume view;
    std::vector<unsigned char> data;

    // the grid-sized volume of `dtype` to hand to the add; null when the tool does not write it
    frog_volume *stage(bool wanted, const frog_volume &grid, int dtype)
    {
        if (!wanted) return nullptr;
        view = grid;
        view.dtype = dtype;
        data.resize((size_t)grid.dims[0] * grid.dims[1] * grid.dims[2] * frog_volume_voxel_bytes(dtype));
        view.data = data.data();
        return &view;
    }

    void write(const std::string &outDir, const char *stem, size_t i) const
    {
        const std::string name = outDir + "/" + stem + std::to_string(i) + ".nii.gz";
        if (frog_volume_write(name.c_str(), &view)) die("cannot write " + name);
    }
};

// Where the time went; the tool adds to the phases as it goes and print() closes its output.
struct PhaseTimes {
    clk::time_point start = clk::now();
    double device_s = 0, write_s = 0, waited_s = 0, setup_s = 0;

    void print(double read_s, int threads) const
    {
        char line[512];
        std::snprintf(line, sizeof line,
                      "read : %.3f s of %d host threads (device waited %.3f s)\ndevice : %.3f s (+ %.3f s set-up)\nwrite : %.3f s\ntotal : %.3f s",
                      read_s, threads, waited_s, device_s, setup_s, write_s, seconds(start));
        std::cout << line << std::endl;
    }
};

#endif
