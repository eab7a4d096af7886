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
#include "group_tool.h"
#include "volume_stream.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

int main(int argc, char *argv[])
{
    PhaseTimes times;
    std::vector<std::string> volumes;
    std::string transformsDir = "transforms", outDir = ".";
    int device = 0, writeTransformed = 0, writeProbabilities = 0;
    long maxLabels = 0;
    double background = 0;
    int a = positional_arguments(argc, argv, 3, { "-td", "-o", "-b", "-ml", "-p", "-wt", "-dev" }, volumes);
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
    ChainArguments transforms;
    const auto inverse = inverse_transforms(transforms, transformsDir, n);
    for (const auto &v : volumes) {
        const VolumeHeader h = peek_header(v);
        if (!h.ok) die("cannot read volume " + v);
        if (h.is_float) die(v + " is a float volume: label maps have an integer type");
    }
    begin_output(outDir, n, "label maps", grid);

    int threads;
    size_t window;
    frog::volume_stream_shape(n, &threads, &window);
    frog::VolumeStream stream(volumes, threads, window);     // reading starts now, beside the device set-up below

    auto t0 = clk::now();
    std::vector<frog_chain *> chains = create_chains(inverse, device);
    frog_labels *acc = nullptr;
    if (frog_labels_create(&grid, (uint32_t)n, (uint32_t)maxLabels, device, &acc)) die(frog_last_error());
    times.setup_s = seconds(t0);

    const size_t total = (size_t)grid.dims[0] * grid.dims[1] * grid.dims[2];
    ReslicedVolume resliced;
    for (size_t i = 0; i < n; i++) {
        double waited = 0;
        frog::VolumeStream::Item &it = stream.get(i, &waited);
        times.waited_s += waited;
        if (!it.file) die("cannot read volume " + volumes[i]);
        frog_volume *out = resliced.stage(writeTransformed, grid, it.view.dtype);
        t0 = clk::now();
        if (frog_labels_add(acc, chains[i], &it.view, background, out)) die(volumes[i] + ": " + frog_last_error());
        times.device_s += seconds(t0);
        stream.release(i);
        frog_chain_destroy(chains[i]);
        chains[i] = nullptr;
        if (out) {
            t0 = clk::now();
            resliced.write(outDir, "transformedLabels", i);
            times.write_s += seconds(t0);
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
    times.device_s += seconds(t0);

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
    times.write_s += seconds(t0);
    if (writeProbabilities) {
        for (uint32_t l = 0; l < n_labels; l++) {
            t0 = clk::now();
            if (frog_labels_probability(acc, values[l], share.data())) die(frog_last_error());
            times.device_s += seconds(t0);
            t0 = clk::now();
            const std::string path = outDir + "/probability_" + std::to_string(values[l]) + ".nii.gz";
            if (frog_volume_write(path.c_str(), &f32)) die("cannot write " + path);
            times.write_s += seconds(t0);
        }
    }
    frog_labels_destroy(acc);
    std::cout << n_labels << " labels" << std::endl;
    times.print(stream.read_seconds(), stream.threads());
    return 0;
}
