// AtlasSegment: multi-atlas segmentation of a target image from a registered group by locally weighted voting (no counterpart
// in the reference; Artaechevarria et al., IEEE TMI 28(8), 2009) or, with -j 1, by joint label fusion (Wang et al., IEEE PAMI
// 35(3), 2013).
//   AtlasSegment bbox.json spacing target image_0 ... image_N-1 -ll labels.txt [-td transformsDir] [-tt target.json] [-o outDir]
//                [-r radius] [-pw power] [-fl floor] [-i interpolation] [-b imageBackground] [-bl labelBackground] [-f fillLabel]
//                [-ml maxLabels] [-p 1] [-wt 1] [-dev n] [-j 1 [-ja alpha] [-jb beta] [-jw 1]]
// The grid is DummyVolumeGenerator's (frog_bbox_grid).  Atlas i is image_i and line i of labels.txt (one label file per line,
// N lines, the list format of AverageImage -ml); both go through the inverse of <transformsDir>/<i>.json (default
// "transforms"), the image exactly as `VolumeTransform image_i dummy.mhd -t transforms/i.json` reslices it (background = its
// minimum unless -b, linear unless -i 0), the label map as `VolumeTransform labels_i dummy.mhd -t transforms/i.json -i 0 -b
// <labelBackground>` does (default 0), with one evaluation of the chain per voxel for the two (frog_wlabels_add).  The target
// goes through the inverse of -tt, the transform `frog -fi/-fd/-r` gives a new subject against the finished group; without
// -tt it is taken to lie in the group's space already.  Every atlas votes for its label with the normalised
// cross-correlation between its image and the target over the (2 radius + 1)^3 patch of the voxel (-r 1..4, default 2),
// raised to -pw (1..8, default 2) and at least -fl (in [0, 1], default 2^-10) before the power.  In outDir:
//   segmentation.nii.gz   per voxel the label with the largest score (ties: the smallest value; -f, default 0, where no atlas
//                         covers the voxel together with the target), as the first of u8, u16, i16, i32, u32 that holds every
//                         label and the fill label
//   confidence.nii.gz     f32 share of the voxel's score that went to that label
//   segmentation.csv      label,voxels,volume_mm3: the voxels of the segmentation per label, counted on the host
//   -p 1                  probability_<value>.nii.gz per label: f32 share of the voxel's score
//   -wt 1                 transformedTarget.nii.gz, transformed<i>.nii.gz and transformedLabels<i>.nii.gz, the files
//                         VolumeTransform would write
//   -j 1                  joint label fusion (frog_jlabels) in place of the weighted vote: at most 32 atlases, -r 1..3; the
//                         weights of a voxel solve the system of the atlases' pairwise patch differences from the target,
//                         raised elementwise to -jb (1..4, default 2) with -ja (> 0, default 0.1) on the diagonal; they sum to 1
//                         and may be negative, so a confidence can exceed 1.  -pw and -fl do not apply and are an error.  The
//                         files keep their names and formats.
//   -jw 1                 with -j 1: weight_<i>.nii.gz per atlas, its f32 weight per voxel
// The segmentation is in the group's space: `VolumeTransform segmentation.nii.gz target -t target.json -i 0` brings it to the
// subject.  Every transform and volume header is checked before anything is written; a float label file is an error.
#include "group_tool.h"
#include "volume_stream.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <map>
#include <string>
#include <vector>

namespace {

const char *USAGE =
    "Usage : AtlasSegment bbox.json spacing target image_0 ... image_N-1 -ll labels.txt [-td transformsDir] [-tt target.json] [-o outDir] "
    "[-r radius=2] [-pw power=2] [-fl floor=0.0009765625] [-i 1] [-b imageBackground] [-bl labelBackground] [-f fillLabel] [-ml maxLabels] "
    "[-p 1] [-wt 1] [-dev n] [-j 1 [-ja alpha=0.1] [-jb beta=2] [-jw 1]]\n"
    "The segmentation is in the group's space: VolumeTransform segmentation.nii.gz target -t target.json -i 0 brings it to the subject.";

// the voxel of an integer volume as a 64-bit value
int64_t label_at(const frog_volume &v, size_t i)
{
    switch (v.dtype) {
    case FROG_V_U8: return ((const uint8_t *)v.data)[i];
    case FROG_V_I8: return ((const int8_t *)v.data)[i];
    case FROG_V_U16: return ((const uint16_t *)v.data)[i];
    case FROG_V_I16: return ((const int16_t *)v.data)[i];
    case FROG_V_U32: return ((const uint32_t *)v.data)[i];
    default: return ((const int32_t *)v.data)[i];
    }
}

} // namespace

int main(int argc, char *argv[])
{
    PhaseTimes times;
    std::vector<std::string> positional, labelFiles;
    std::string transformsDir = "transforms", outDir = ".", labelList, targetTransform;
    int device = 0, writeTransformed = 0, writeProbabilities = 0, interpolation = 1, joint = 0, writeWeights = 0;
    bool votingOption = false, jointOption = false;         // -pw or -fl given; -ja, -jb or -jw given
    long radius = 2, power = 2, maxLabels = 0, beta = 2;
    double alpha = 0.1;
    long long fillLabel = 0;
    float floor = 0.0009765625f;
    double labelBackground = 0;
    BackgroundLevel background;
    int a = positional_arguments(argc, argv, 3, { "-ll", "-td", "-tt", "-o", "-r", "-pw", "-fl", "-i", "-b", "-bl", "-f", "-ml", "-p", "-wt", "-dev", "-j", "-ja", "-jb", "-jw" }, positional);
    for (; a < argc; a += 2) {
        const char *key = argv[a], *value = a + 1 < argc ? argv[a + 1] : "";
        if (std::strcmp(key, "-ll") == 0) labelList = value;
        else if (std::strcmp(key, "-td") == 0) transformsDir = value;
        else if (std::strcmp(key, "-tt") == 0) targetTransform = value;
        else if (std::strcmp(key, "-o") == 0) outDir = value;
        else if (std::strcmp(key, "-r") == 0) radius = atol(value);
        else if (std::strcmp(key, "-pw") == 0) { power = atol(value); votingOption = true; }
        else if (std::strcmp(key, "-fl") == 0) { floor = (float)atof(value); votingOption = true; }
        else if (std::strcmp(key, "-j") == 0) joint = atoi(value);
        else if (std::strcmp(key, "-ja") == 0) { alpha = atof(value); jointOption = true; }
        else if (std::strcmp(key, "-jb") == 0) { beta = atol(value); jointOption = true; }
        else if (std::strcmp(key, "-jw") == 0) { writeWeights = atoi(value); jointOption = true; }
        else if (std::strcmp(key, "-i") == 0) interpolation = atoi(value);
        else if (std::strcmp(key, "-b") == 0) background.parse(value);
        else if (std::strcmp(key, "-bl") == 0) labelBackground = (float)atof(value);  // a float, as VolumeTransform parses -b
        else if (std::strcmp(key, "-f") == 0) fillLabel = atoll(value);
        else if (std::strcmp(key, "-ml") == 0) maxLabels = atol(value);
        else if (std::strcmp(key, "-p") == 0) writeProbabilities = atoi(value);
        else if (std::strcmp(key, "-wt") == 0) writeTransformed = atoi(value);
        else if (std::strcmp(key, "-dev") == 0) device = atoi(value);
        else die(std::string("unknown option ") + key);
    }
    if (argc < 5 || positional.size() < 2 || labelList.empty()) {
        std::cout << USAGE << std::endl;
        return 1;
    }
    const std::string target = positional[0];
    const std::vector<std::string> images(positional.begin() + 1, positional.end());
    const size_t n = images.size();
    if (joint) {
        if (votingOption) die("-pw and -fl belong to the weighted vote: they do not go with -j 1");
        if (n > 32) die("-j 1 : at most 32 atlases");
        if (radius < 1 || radius > 3) die("-r : a radius from 1 to 3 with -j 1");
        if (beta < 1 || beta > 4) die("-jb : a beta from 1 to 4");
        if (!(std::isfinite(alpha) && alpha > 0)) die("-ja : a finite alpha above 0");
    } else if (jointOption) {
        die("-ja, -jb and -jw belong to joint label fusion: they need -j 1");
    }
    if (radius < 1 || radius > 4) die("-r : a radius from 1 to 4");
    if (power < 1 || power > 8) die("-pw : a power from 1 to 8");
    if (!(floor >= 0.0f && floor <= 1.0f)) die("-fl : a floor in [0, 1]");
    if (maxLabels < 0 || maxLabels > 65536) die("-ml : 1 to 65536 labels");
    if (!std::isfinite(labelBackground)) die("-bl : a finite label");
    if (!read_list(labelList, labelFiles)) die("cannot read the label list " + labelList);
    if (labelFiles.size() != n) die(labelList + " holds " + std::to_string(labelFiles.size()) + " label maps for " + std::to_string(n) + " images");

    // ---- everything is checked before the first output: the grid, every transform, every volume header
    frog_volume grid;
    if (frog_bbox_grid(argv[1], atof(argv[2]), &grid)) die(std::string("cannot read a bounding box from ") + argv[1] + " (or spacing " + argv[2] + " is not positive)");
    ChainArguments transforms, targetTransforms;
    const auto inverse = inverse_transforms(transforms, transformsDir, n);
    std::string error;
    if (!targetTransform.empty() && !targetTransforms.add(targetTransform.c_str(), true, error)) die(error);
    if (!peek_header(target).ok) die("cannot read volume " + target);
    for (const auto &v : images) if (!peek_header(v).ok) die("cannot read volume " + v);
    for (const auto &l : labelFiles) {
        const VolumeHeader h = peek_header(l);
        if (!h.ok) die("cannot read label map " + l);
        if (h.is_float) die(l + " is a float volume: label maps have an integer type");
    }
    begin_output(outDir, n, "atlases", grid);

    int threads;
    size_t window;
    frog::volume_stream_shape(n, &threads, &window);
    threads = std::max(1, threads / 2);                      // the label maps have readers of their own
    frog::VolumeStream stream(images, threads, window);      // reading starts now, beside the device set-up below
    frog::VolumeStream labelStream(labelFiles, threads, window);
    frog::VolumeStream targetStream({ target }, 1, 1);

    auto t0 = clk::now();
    std::vector<frog_chain *> chains = create_chains(inverse, device);
    frog_chain *targetChain = nullptr;                       // no -tt: a chain without links, the identity
    if (frog_chain_create(targetTransforms.links.data(), (uint32_t)targetTransforms.links.size(), device, &targetChain)) die(target + ": " + frog_last_error());
    // one of the two accumulators; after create their calls take the same arguments
    frog_wlabels *acc = nullptr;
    frog_jlabels *jacc = nullptr;
    if (joint ? frog_jlabels_create(&grid, (uint32_t)n, (uint32_t)maxLabels, (uint32_t)radius, (uint32_t)beta, alpha, writeWeights, device, &jacc)
              : frog_wlabels_create(&grid, (uint32_t)n, (uint32_t)maxLabels, (uint32_t)radius, (uint32_t)power, floor, device, &acc))
        die(frog_last_error());
    times.setup_s = seconds(t0);

    const size_t total = (size_t)grid.dims[0] * grid.dims[1] * grid.dims[2];
    ReslicedVolume resliced, reslicedLabels;
    {
        double waited = 0;
        frog::VolumeStream::Item &it = targetStream.get(0, &waited);
        times.waited_s += waited;
        if (!it.file) die("cannot read volume " + target);
        frog_volume *out = resliced.stage(writeTransformed, grid, it.view.dtype);
        t0 = clk::now();
        if (joint ? frog_jlabels_target(jacc, targetChain, &it.view, interpolation, background.of(it.lo), out)
                  : frog_wlabels_target(acc, targetChain, &it.view, interpolation, background.of(it.lo), out))
            die(target + ": " + frog_last_error());
        times.device_s += seconds(t0);
        targetStream.release(0);
        frog_chain_destroy(targetChain);
        if (out) {
            t0 = clk::now();
            const std::string name = outDir + "/transformedTarget.nii.gz";
            if (frog_volume_write(name.c_str(), out)) die("cannot write " + name);
            times.write_s += seconds(t0);
        }
    }
    for (size_t i = 0; i < n; i++) {
        double waited = 0;
        frog::VolumeStream::Item &it = stream.get(i, &waited);
        times.waited_s += waited;
        if (!it.file) die("cannot read volume " + images[i]);
        frog::VolumeStream::Item &lt = labelStream.get(i, &waited);
        times.waited_s += waited;
        if (!lt.file) die("cannot read label map " + labelFiles[i]);
        frog_volume *out = resliced.stage(writeTransformed, grid, it.view.dtype);
        frog_volume *lout = reslicedLabels.stage(writeTransformed, grid, lt.view.dtype);
        t0 = clk::now();
        if (joint ? frog_jlabels_add(jacc, chains[i], &it.view, &lt.view, interpolation, background.of(it.lo), labelBackground, out, lout)
                  : frog_wlabels_add(acc, chains[i], &it.view, &lt.view, interpolation, background.of(it.lo), labelBackground, out, lout))
            die(images[i] + ", " + labelFiles[i] + ": " + frog_last_error());
        times.device_s += seconds(t0);
        stream.release(i);
        labelStream.release(i);
        frog_chain_destroy(chains[i]);
        chains[i] = nullptr;
        if (out) {
            t0 = clk::now();
            resliced.write(outDir, "transformed", i);
            reslicedLabels.write(outDir, "transformedLabels", i);
            times.write_s += seconds(t0);
        }
    }
    t0 = clk::now();
    uint32_t n_labels = 0;
    if (joint ? frog_jlabels_finish(jacc, &n_labels) : frog_wlabels_finish(acc, &n_labels)) die(frog_last_error());
    std::vector<int64_t> values(n_labels);
    if (joint ? frog_jlabels_values(jacc, values.data()) : frog_wlabels_values(acc, values.data())) die(frog_last_error());
    std::vector<int64_t> range = values;                     // the segmentation's type holds the fill label too
    range.insert(std::lower_bound(range.begin(), range.end(), (int64_t)fillLabel), (int64_t)fillLabel);
    const int dtype = fused_type(range);
    if (dtype < 0) die("no integer type of at most 32 bits holds every label from " + std::to_string(range.front()) + " to " + std::to_string(range.back()));
    std::vector<unsigned char> fused(total * frog_volume_voxel_bytes(dtype));
    std::vector<float> share(total);
    frog_volume label = grid;
    label.dtype = dtype;
    label.data = fused.data();
    if (joint ? frog_jlabels_fused(jacc, fillLabel, &label, share.data()) : frog_wlabels_fused(acc, fillLabel, &label, share.data())) die(frog_last_error());
    times.device_s += seconds(t0);

    t0 = clk::now();
    const std::string labels_path = outDir + "/segmentation.nii.gz", confidence_path = outDir + "/confidence.nii.gz", csv_path = outDir + "/segmentation.csv";
    if (frog_volume_write(labels_path.c_str(), &label)) die("cannot write " + labels_path);
    frog_volume f32 = grid;
    f32.dtype = FROG_V_F32;
    f32.data = share.data();
    if (frog_volume_write(confidence_path.c_str(), &f32)) die("cannot write " + confidence_path);
    std::map<int64_t, uint64_t> voxels;
    for (size_t v = 0; v < total; v++) voxels[label_at(label, v)]++;
    FILE *csv = std::fopen(csv_path.c_str(), "w");
    if (!csv) die("cannot write " + csv_path);
    std::fprintf(csv, "label,voxels,volume_mm3\n");
    const double voxel_mm3 = grid.spacing[0] * grid.spacing[1] * grid.spacing[2];
    for (const auto &row : voxels)
        std::fprintf(csv, "%lld,%llu,%.17g\n", (long long)row.first, (unsigned long long)row.second, (double)row.second * voxel_mm3);
    if (std::fclose(csv) != 0) die("cannot write " + csv_path);
    times.write_s += seconds(t0);
    if (writeProbabilities) {
        for (uint32_t l = 0; l < n_labels; l++) {
            t0 = clk::now();
            if (joint ? frog_jlabels_probability(jacc, values[l], share.data()) : frog_wlabels_probability(acc, values[l], share.data())) die(frog_last_error());
            times.device_s += seconds(t0);
            t0 = clk::now();
            const std::string path = outDir + "/probability_" + std::to_string(values[l]) + ".nii.gz";
            if (frog_volume_write(path.c_str(), &f32)) die("cannot write " + path);
            times.write_s += seconds(t0);
        }
    }
    for (size_t i = 0; joint && writeWeights && i < n; i++) {
        t0 = clk::now();
        if (frog_jlabels_weight(jacc, (uint32_t)i, share.data())) die(frog_last_error());
        times.device_s += seconds(t0);
        t0 = clk::now();
        const std::string path = outDir + "/weight_" + std::to_string(i) + ".nii.gz";
        if (frog_volume_write(path.c_str(), &f32)) die("cannot write " + path);
        times.write_s += seconds(t0);
    }
    frog_wlabels_destroy(acc);
    frog_jlabels_destroy(jacc);
    std::cout << n_labels << " labels" << std::endl;
    times.print(stream.read_seconds() + labelStream.read_seconds() + targetStream.read_seconds(), stream.threads() + labelStream.threads() + 1);
    return 0;
}
