// FuseLabels: majority-vote fusion of a registered group's label maps in one process (the reference has no counterpart: it
// stops at one `VolumeTransform -i 0` per image and leaves the N resliced label volumes to a script).
//   FuseLabels bbox.json spacing labels_0 ... labels_N-1 [-td transformsDir] [-o outDir] [-b background] [-ml maxLabels]
//              [-p 1] [-wt 1] [-dev n]
// The grid is DummyVolumeGenerator's (frog_bbox_grid); label map i goes through the inverse of <transformsDir>/<i>.json
// (default "transforms") with nearest-neighbour interpolation exactly as `VolumeTransform labels_i dummy.mhd -t
// transforms/i.json -i 0 -b <background>` does it (same device code; background 0 unless -b) and votes on the device
// (frog_labels_add).  In outDir:
//   labels.nii.gz       per voxel the label with the most votes (ties: the smallest value), as the first of u8, u16, i16, i32,
//                       u32 that holds every label
//   agreement.nii.gz    f32 share of the images that voted for it
//   labels.csv          label,voxels,mean_volume_mm3,group_dice: per label the votes summed over the voxels, that times the
//                       voxel volume / N, and the pooled pairwise Dice overlap across the group, 2 pairs / ((N - 1) voxels)
//                       (include/frog_chain.h; nan for N = 1)
//   -p 1                probability_<value>.nii.gz per label: f32 share of the images that carry it
//   -wt 1               transformedLabels<i>.nii.gz, the file VolumeTransform -i 0 would write
// Every transform and volume header is checked before anything is written; a float label file is an error.  Volumes are
// read and inflated on host threads ahead of the device (volume_stream.h).
#include "tool_common.h"
#include "volume_stream.h"

#include <sys/stat.h>
#include <cerrno>
#include <zlib.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

namespace {

bool has_suffix(const std::string &path, const char *s)
{
    const size_t n = std::strlen(s);
    return path.size() >= n && path.compare(path.size() - n, n, s) == 0;
}

// The header of a label volume, without inflating its data: 0 it does not parse, 1 an integer volume, 2 a float one.
// NIfTI-1: sizeof_hdr and the datatype code at byte 70 (16 FLOAT32, 64 FLOAT64); MetaImage: DimSize present, ElementType.
int label_header(const std::string &path)
{
    if (has_suffix(path, ".mhd") || has_suffix(path, ".mha")) {
        uint32_t d[3]; double sp[3], o[3];
        if (frog_volume_geometry(path.c_str(), d, sp, o) != FROG_OK) return 0;
        FILE *f = std::fopen(path.c_str(), "rb");
        if (!f) return 0;
        char line[512];
        int kind = 1;
        while (std::fgets(line, sizeof line, f)) {
            if (std::strncmp(line, "ElementType", 11) == 0 && (std::strstr(line, "MET_FLOAT") || std::strstr(line, "MET_DOUBLE"))) kind = 2;
            if (std::strncmp(line, "ElementDataFile", 15) == 0) break;
        }
        std::fclose(f);
        return kind;
    }
    if (!has_suffix(path, ".nii") && !has_suffix(path, ".nii.gz")) return 0;
    gzFile f = gzopen(path.c_str(), "rb");
    if (!f) return 0;
    unsigned char h[72];
    const bool ok = gzread(f, h, sizeof h) == (int)sizeof h;
    gzclose(f);
    int32_t n = 0;
    int16_t datatype = 0;
    std::memcpy(&n, h, sizeof n);
    std::memcpy(&datatype, h + 70, sizeof datatype);
    if (!ok || n != 348) return 0;
    return datatype == 16 || datatype == 64 ? 2 : 1;
}

// the first of u8, u16, i16, i32, u32 that holds every value; -1 if none does
int fused_type(const std::vector<int64_t> &values)
{
    int64_t lo = 0, hi = 0;
    if (!values.empty()) { lo = values.front(); hi = values.back(); }         // ascending
    const struct { int dtype; int64_t lo, hi; } types[] = {
        { FROG_V_U8, 0, 255 }, { FROG_V_U16, 0, 65535 }, { FROG_V_I16, -32768, 32767 },
        { FROG_V_I32, -2147483647LL - 1, 2147483647LL }, { FROG_V_U32, 0, 4294967295LL } };
    for (const auto &t : types) if (t.lo <= lo && hi <= t.hi) return t.dtype;
    return -1;
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
    int device = 0, writeTransformed = 0, writeProbabilities = 0;
    long maxLabels = 0;
    double background = 0;
    auto is_flag = [](const char *a) {
        for (const char *f : { "-td", "-o", "-b", "-ml", "-p", "-wt", "-dev" }) if (std::strcmp(a, f) == 0) return true;
        return false;
    };
    int a = 3;
    for (; a < argc && !is_flag(argv[a]); a++) volumes.push_back(argv[a]);
    for (; a < argc; a += 2) {
        const char *key = argv[a], *value = a + 1 < argc ? argv[a + 1] : "";
        if (std::strcmp(key, "-td") == 0) transformsDir = value;
        else if (std::strcmp(key, "-o") == 0) outDir = value;
        else if (std::strcmp(key, "-b") == 0) background = (float)atof(value);       // a float, as VolumeTransform parses -b
        else if (std::strcmp(key, "-ml") == 0) maxLabels = atol(value);
        else if (std::strcmp(key, "-p") == 0) writeProbabilities = atoi(value);
        else if (std::strcmp(key, "-wt") == 0) writeTransformed = atoi(value);
        else if (std::strcmp(key, "-dev") == 0) device = atoi(value);
        else die(std::string("unknown option ") + key);
    }
    if (argc < 4 || volumes.empty()) {
        std::cout << "Usage : FuseLabels bbox.json spacing labels_0 ... labels_N-1 [-td transformsDir] [-o outDir] [-b background] "
                     "[-ml maxLabels] [-p 1] [-wt 1] [-dev n]" << std::endl;
        return 1;
    }
    const size_t n = volumes.size();
    if (maxLabels < 0 || maxLabels > 65536) die("-ml : 1 to 65536 labels");
    if (n > 65535) die("at most 65535 label volumes");

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
    for (const auto &v : volumes) {
        const int kind = label_header(v);
        if (kind == 0) die("cannot read volume " + v);
        if (kind == 2) die(v + " is a float volume: label maps have an integer type");
    }
    if (mkdir(outDir.c_str(), 0755) != 0 && errno != EEXIST) die("cannot create " + outDir);
    std::cout << n << " label maps, grid " << grid.dims[0] << " x " << grid.dims[1] << " x " << grid.dims[2] << " (spacing " << grid.spacing[0]
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
    frog_labels *acc = nullptr;
    if (frog_labels_create(&grid, (uint32_t)n, (uint32_t)maxLabels, device, &acc)) die(frog_last_error());
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
        if (frog_labels_add(acc, chains[i], &it.view, background, out)) die(volumes[i] + ": " + frog_last_error());
        device_s += seconds(t0);
        stream.release(i);
        frog_chain_destroy(chains[i]);
        chains[i] = nullptr;
        if (out) {
            t0 = clk::now();
            const std::string name = outDir + "/transformedLabels" + std::to_string(i) + ".nii.gz";
            if (frog_volume_write(name.c_str(), out)) die("cannot write " + name);
            write_s += seconds(t0);
        }
    }
    t0 = clk::now();
    uint32_t n_labels = 0;
    if (frog_labels_finish(acc, &n_labels)) die(frog_last_error());
    std::vector<int64_t> values(n_labels);
    std::vector<uint64_t> voxels(n_labels), pairs(n_labels);
    if (frog_labels_table(acc, values.data(), voxels.data(), pairs.data())) die(frog_last_error());
    const int dtype = fused_type(values);
    if (dtype < 0) die("no integer type of at most 32 bits holds every label from " + std::to_string(values.front()) + " to " + std::to_string(values.back()));
    std::vector<unsigned char> fused(total * frog_volume_voxel_bytes(dtype));
    std::vector<float> share(total);
    frog_volume label = grid;
    label.dtype = dtype;
    label.data = fused.data();
    if (frog_labels_fused(acc, &label, share.data())) die(frog_last_error());
    device_s += seconds(t0);

    t0 = clk::now();
    const std::string labels_path = outDir + "/labels.nii.gz", agreement_path = outDir + "/agreement.nii.gz", csv_path = outDir + "/labels.csv";
    if (frog_volume_write(labels_path.c_str(), &label)) die("cannot write " + labels_path);
    frog_volume f32 = grid;
    f32.dtype = FROG_V_F32;
    f32.data = share.data();
    if (frog_volume_write(agreement_path.c_str(), &f32)) die("cannot write " + agreement_path);
    FILE *csv = std::fopen(csv_path.c_str(), "w");
    if (!csv) die("cannot write " + csv_path);
    std::fprintf(csv, "label,voxels,mean_volume_mm3,group_dice\n");
    const double voxel_mm3 = grid.spacing[0] * grid.spacing[1] * grid.spacing[2];
    for (uint32_t l = 0; l < n_labels; l++) {
        const double dice = n > 1 ? 2.0 * (double)pairs[l] / ((double)(n - 1) * (double)voxels[l]) : std::nan("");
        std::fprintf(csv, "%lld,%llu,%.17g,%.17g\n", (long long)values[l], (unsigned long long)voxels[l],
                     (double)voxels[l] * voxel_mm3 / (double)n, dice);
    }
    if (std::fclose(csv) != 0) die("cannot write " + csv_path);
    write_s += seconds(t0);
    if (writeProbabilities) {
        for (uint32_t l = 0; l < n_labels; l++) {
            t0 = clk::now();
            if (frog_labels_probability(acc, values[l], share.data())) die(frog_last_error());
            device_s += seconds(t0);
            t0 = clk::now();
            const std::string path = outDir + "/probability_" + std::to_string(values[l]) + ".nii.gz";
            if (frog_volume_write(path.c_str(), &f32)) die("cannot write " + path);
            write_s += seconds(t0);
        }
    }
    frog_labels_destroy(acc);
    std::cout << n_labels << " labels" << std::endl;
    char line[512];
    std::snprintf(line, sizeof line,
                  "read : %.3f s of %d host threads (device waited %.3f s)\ndevice : %.3f s (+ %.3f s set-up)\nwrite : %.3f s\ntotal : %.3f s",
                  stream.read_seconds(), stream.threads(), waited_s, device_s, setup_s, write_s, seconds(t_start));
    std::cout << line << std::endl;
    return 0;
}
