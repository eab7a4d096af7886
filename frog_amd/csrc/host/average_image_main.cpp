// AverageImage: the group's average and stdev images in one process -- what transform.sh (and FROG.py -a) computes with
// DummyVolumeGenerator, one VolumeTransform per image and AverageVolumes, without writing and re-reading N volumes and
// without N + 2 HIP runtime starts.
//   AverageImage bbox.json spacing v_0 ... v_{N-1} [-td transformsDir] [-o outDir] [-i interpolation] [-b background]
//                [-wt 1] [-dev n]
// The grid is DummyVolumeGenerator's (frog_bbox_grid); image i is resliced through the inverse of <transformsDir>/<i>.json
// (default "transforms"; -j and sidecar forms) exactly as `VolumeTransform v_i dummy.mhd -t transforms/i.json` does it
// (same device code; background = the image's minimum unless -b, linear unless -i 0), converted to its own type and added
// on the device (frog_average_add) in image order, so average.nii.gz and stdev.nii.gz in outDir are AverageVolumes' files
// bit for bit.  -wt 1 also writes transformed<i>.nii.gz, the file transform.sh leaves behind.  Every transform and volume
// header is checked before anything is written.  Volumes are read and inflated on host threads ahead of the device, a
// bounded number at a time (volume_stream.h).
#include "tool_common.h"
#include "volume_stream.h"

#include <sys/stat.h>
#include <cerrno>
#include <zlib.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

namespace {

// the header of a volume parses (NIfTI-1: sizeof_hdr; MetaImage: DimSize present), without inflating its data
bool header_ok(const std::string &path)
{
    auto has_suffix = [&](const char *s) { const size_t n = std::strlen(s); return path.size() >= n && path.compare(path.size() - n, n, s) == 0; };
    if (has_suffix(".mhd") || has_suffix(".mha")) {
        uint32_t d[3]; double sp[3], o[3];
        return frog_volume_geometry(path.c_str(), d, sp, o) == FROG_OK;
    }
    if (!has_suffix(".nii") && !has_suffix(".nii.gz")) return false;
    gzFile f = gzopen(path.c_str(), "rb");
    if (!f) return false;
    int32_t n = 0;
    const bool ok = gzread(f, &n, sizeof n) == (int)sizeof n && n == 348;
    gzclose(f);
    return ok;
}

} // namespace

int main(int argc, char *argv[])
{
    using clk = std::chrono::steady_clock;
    const auto t_start = clk::now();
    auto seconds = [](clk::time_point a) { return std::chrono::duration<double>(clk::now() - a).count(); };
    // reader threads may still be inflating: leave without running static destructors under them
    auto die = [](const std::string &what) { std::cout << "Error : " << what << std::endl; std::_Exit(1); };
    std::vector<std::string> volumes;
    std::string transformsDir = "transforms", outDir = ".";
    int interpolation = 1, device = 0, writeTransformed = 0;
    BackgroundLevel background;
    auto is_flag = [](const char *a) {
        for (const char *f : { "-td", "-o", "-i", "-b", "-wt", "-dev" }) if (std::strcmp(a, f) == 0) return true;
        return false;
    };
    int a = 3;
    for (; a < argc && !is_flag(argv[a]); a++) volumes.push_back(argv[a]);
    for (; a < argc; a += 2) {
        const char *key = argv[a], *value = a + 1 < argc ? argv[a + 1] : "";
        if (std::strcmp(key, "-td") == 0) transformsDir = value;
        else if (std::strcmp(key, "-o") == 0) outDir = value;
        else if (std::strcmp(key, "-i") == 0) interpolation = atoi(value);
        else if (std::strcmp(key, "-b") == 0) background.parse(value);
        else if (std::strcmp(key, "-wt") == 0) writeTransformed = atoi(value);
        else if (std::strcmp(key, "-dev") == 0) device = atoi(value);
        else die(std::string("unknown option ") + key);
    }
    if (argc < 4 || volumes.empty()) {
        std::cout << "Usage : AverageImage bbox.json spacing image_0 ... image_N-1 [-td transformsDir] [-o outDir] [-i interpolation] "
                     "[-b background] [-wt 1] [-dev n]" << std::endl;
        return 1;
    }
    const size_t n = volumes.size();

    // ---- everything is checked before the first output: the grid, every transform, every volume header
    frog_volume grid;
    if (frog_bbox_grid(argv[1], atof(argv[2]), &grid)) die(std::string("cannot read a bounding box from ") + argv[1] + " (or spacing " + argv[2] + " is not positive)");
    ChainArguments transforms;                              // owns the files; every image has a chain of its own
    std::vector<std::vector<frog_chain_link>> inverse(n);
    for (size_t i = 0; i < n; i++) {
        const std::string path = transformsDir + "/" + std::to_string(i) + ".json";
        frog_transform_file *f = transforms.read(path.c_str());
        if (!f) die("cannot read transform " + path);
        const uint32_t nl = frog_transform_num_links(f);
        inverse[i].resize(nl);
        if (frog_chain_invert_links(frog_transform_links(f), nl, inverse[i].data())) die(path + ": " + frog_last_error());
    }
    for (const auto &v : volumes) if (!header_ok(v)) die("cannot read volume " + v);
    if (mkdir(outDir.c_str(), 0755) != 0 && errno != EEXIST) die("cannot create " + outDir);
    std::cout << n << " images, grid " << grid.dims[0] << " x " << grid.dims[1] << " x " << grid.dims[2] << " (spacing " << grid.spacing[0]
              << ", origin " << grid.origin[0] << " " << grid.origin[1] << " " << grid.origin[2] << ")" << std::endl;

    int threads;
    size_t window;
    frog::volume_stream_shape(n, &threads, &window);
    frog::VolumeStream stream(volumes, threads, window);     // reading starts now, beside the device set-up below

    double device_s = 0, write_s = 0, waited_s = 0;
    auto t0 = clk::now();
    std::vector<frog_chain *> chains(n, nullptr);
    for (size_t i = 0; i < n; i++)
        if (frog_chain_create(inverse[i].data(), (uint32_t)inverse[i].size(), device, &chains[i])) die("transform " + std::to_string(i) + ": " + frog_last_error());
    frog_average *avg = nullptr;
    if (frog_average_create(&grid, (uint32_t)n, device, &avg)) die(frog_last_error());
    const double setup_s = seconds(t0);

    const size_t total = (size_t)grid.dims[0] * grid.dims[1] * grid.dims[2];
    std::vector<unsigned char> resliced_data;
    for (size_t i = 0; i < n; i++) {
        double waited = 0;
        frog::VolumeStream::Item &it = stream.get(i, &waited);
        waited_s += waited;
        if (!it.file) die("cannot read volume " + volumes[i]);
        frog_volume resliced = grid, *out = nullptr;
        if (writeTransformed) {
            resliced.dtype = it.view.dtype;
            resliced_data.resize(total * frog_volume_voxel_bytes(it.view.dtype));
            resliced.data = resliced_data.data();
            out = &resliced;
        }
        t0 = clk::now();
        if (frog_average_add(avg, chains[i], &it.view, interpolation, background.of(it.lo), out))
            die(volumes[i] + ": " + frog_last_error());
        device_s += seconds(t0);
        stream.release(i);
        frog_chain_destroy(chains[i]);
        chains[i] = nullptr;
        if (out) {
            t0 = clk::now();
            const std::string name = outDir + "/transformed" + std::to_string(i) + ".nii.gz";
            if (frog_volume_write(name.c_str(), out)) die("cannot write " + name);
            write_s += seconds(t0);
        }
    }
    std::vector<float> mean(total), stdev(total);
    t0 = clk::now();
    if (frog_average_finish(avg, mean.data(), stdev.data())) die(frog_last_error());
    device_s += seconds(t0);
    frog_average_destroy(avg);

    t0 = clk::now();
    grid.dtype = FROG_V_F32;
    for (auto [name, data] : { std::make_pair("average.nii.gz", mean.data()), std::make_pair("stdev.nii.gz", stdev.data()) }) {
        grid.data = data;
        const std::string path = outDir + "/" + name;
        if (frog_volume_write(path.c_str(), &grid)) die("cannot write " + path);
    }
    write_s += seconds(t0);
    char line[512];
    std::snprintf(line, sizeof line,
                  "read : %.3f s of %d host threads (device waited %.3f s)\ndevice : %.3f s (+ %.3f s set-up)\nwrite : %.3f s\ntotal : %.3f s",
                  stream.read_seconds(), stream.threads(), waited_s, device_s, setup_s, write_s, seconds(t_start));
    std::cout << line << std::endl;
    return 0;
}
