// FuseLabels: majority-vote fusion of a registered group's label maps in one process (the reference has no counterpart: it
// stops at one `VolumeTransform -i 0` per image and leaves the N resliced label volumes to a script).
//   FuseLabels bbox.json spacing labels_0 ... labels_N-1 [-td transformsDir] [-o outDir] [-b background] [-ml maxLabels]
//              [-p 1] [-wt 1] [-dev n] [-s 1 [-sp p0] [-st tol] [-si maxIter] [-sr 0|1]] [-d 1 [-dp percentile] [-dr 0|1]]
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
//   -s 1                STAPLE beside the vote (frog_staple, include/frog_chain.h: an EM estimate that weights every image's
//                       vote by its estimated confusion matrix; at most 256 labels and 4096 images).  The resliced label
//                       map of every image goes from frog_labels_add to frog_staple_add: one chain evaluation per image.
//                       -sp: the starting diagonal of the confusion matrices (0.99); -st: the EM stops when no entry
//                       changes by more (1e-6); -si: the most iterations (50); -sr 1: only the voxels on which the images
//                       disagree take part.  It adds
//     staple.nii.gz             per voxel the most probable label, typed as labels.nii.gz
//     staple_confidence.nii.gz  its f32 probability
//     staple.csv                label,prior,voxels,volume_mm3: the prior of the EM, the voxels of staple.nii.gz, their volume
//     performance.csv           image,file,accuracy,accuracy_robust_z,sensitivity_<value>...: accuracy = sum_l S[i][l][l] /
//                               sum_l T[l] (u64 sums, one f64 division), its robust z across the group by quality.csv's rule
//                               ((a - median) / (1.4826 MAD), 0 where the MAD is 0), and theta[i][l][l] per label
//     -p 1                      staple_probability_<value>.nii.gz per label
//                       and a line "staple : <iterations> iterations, change <c>, <A> active voxels".
//   -d 1                surface distances of every image to the consensus (frog_surface, include/frog_chain.h: an exact
//                       Euclidean distance transform on the device), after everything above is written.  The consensus is
//                       labels.nii.gz (-dr 0) or staple.nii.gz (-dr 1, which needs -s 1); every value of the table except the
//                       background (-b) is measured, at most 256.  The label maps are streamed a second time through
//                       re-created chains.  -dp: the percentile p, 1 to 100 (95).  It adds, every floating-point column
//                       printed with %.17g and in the unit of the spacing:
//     surface.csv               image,file,label,surface_voxels,reference_surface_voxels,hausdorff,hausdorff_<p>,assd: one row
//                               per image and label; nan where the label has no surface in the image or in the consensus
//     surface_images.csv        image,file,labels_measured,mean_assd,mean_assd_robust_z,max_hausdorff: over the labels with
//                               both surfaces; the robust z as performance.csv's, nan for an image with nothing measured
//     surface_labels.csv        label,images_measured,mean_assd,max_hausdorff,mean_hausdorff_<p>: over the images
//                       A mean is the sum in ascending order of the labels (of the images) from +0.0, over their number.
//                       And a line "surface : <seconds> s" after the phase times.
// Every option, transform and volume header is checked before anything is written; a float label file is an error.  Volumes are
// read and inflated on host threads ahead of the device (volume_stream.h).
#include "group_tool.h"
#include "volume_stream.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

namespace {

// the median of a non-empty list: the middle value, or the mean of the middle two (as quality.csv's)
double median(std::vector<double> v)
{
    std::sort(v.begin(), v.end());
    const size_t n = v.size();
    return n % 2 ? v[n / 2] : (v[n / 2 - 1] + v[n / 2]) / 2.0;
}

// What a reader sees of a row, by the three lines of include/frog_chain.h; all nan when either surface is empty.
struct SurfaceMetrics {
    double hausdorff = NAN, hausdorff_p = NAN, assd = NAN;
};

SurfaceMetrics surface_metrics(const frog_surface_row &r)
{
    SurfaceMetrics m;
    if (!r.n_a || !r.n_b) return m;
    m.hausdorff = (double)std::max(r.max_ab, r.max_ba) * 0x1p-16;
    m.hausdorff_p = (double)std::max(r.pct_ab, r.pct_ba) * 0x1p-16;
    m.assd = ((double)(r.sum_ab + r.sum_ba) / (double)(r.n_a + r.n_b)) * 0x1p-16;
    return m;
}

// %.17g, and nan without a sign
std::string g17(double v)
{
    if (std::isnan(v)) return "nan";
    char text[40];
    std::snprintf(text, sizeof text, "%.17g", v);
    return text;
}

// the sum of the values one by one from +0.0 over their number; nan for none
double mean_in_order(const std::vector<double> &v)
{
    double total = 0.0;
    for (const double x : v) total = total + x;
    return v.empty() ? NAN : total / (double)v.size();
}

} // namespace

int main(int argc, char *argv[])
{
    PhaseTimes times;
    std::vector<std::string> volumes;
    std::string transformsDir = "transforms", outDir = ".";
    int device = 0, writeTransformed = 0, writeProbabilities = 0, staple = 0, stapleRestrict = 0, surface = 0, surfaceReference = 0;
    long maxLabels = 0, stapleIterations = 50, surfacePercentile = 95;
    double background = 0, stapleP0 = 0.99, stapleTol = 1e-6;
    bool stapleOption = false;                              // one of -sp, -st, -si, -sr was given
    bool surfaceOption = false;                             // one of -dp, -dr was given
    int a = positional_arguments(argc, argv, 3, { "-td", "-o", "-b", "-ml", "-p", "-wt", "-dev", "-s", "-sp", "-st", "-si", "-sr", "-d", "-dp", "-dr" }, volumes);
    for (; a < argc; a += 2) {
        const char *key = argv[a], *value = a + 1 < argc ? argv[a + 1] : "";
        if (std::strcmp(key, "-td") == 0) transformsDir = value;
        else if (std::strcmp(key, "-o") == 0) outDir = value;
        else if (std::strcmp(key, "-b") == 0) background = (float)atof(value);       // a float, as VolumeTransform parses -b
        else if (std::strcmp(key, "-ml") == 0) maxLabels = atol(value);
        else if (std::strcmp(key, "-p") == 0) writeProbabilities = atoi(value);
        else if (std::strcmp(key, "-wt") == 0) writeTransformed = atoi(value);
        else if (std::strcmp(key, "-dev") == 0) device = atoi(value);
        else if (std::strcmp(key, "-s") == 0) staple = atoi(value);
        else if (std::strcmp(key, "-sp") == 0) { stapleP0 = atof(value); stapleOption = true; }
        else if (std::strcmp(key, "-st") == 0) { stapleTol = atof(value); stapleOption = true; }
        else if (std::strcmp(key, "-si") == 0) { stapleIterations = atol(value); stapleOption = true; }
        else if (std::strcmp(key, "-sr") == 0) { stapleRestrict = atoi(value); stapleOption = true; }
        else if (std::strcmp(key, "-d") == 0) surface = atoi(value);
        else if (std::strcmp(key, "-dp") == 0) { surfacePercentile = atol(value); surfaceOption = true; }
        else if (std::strcmp(key, "-dr") == 0) { surfaceReference = atoi(value); surfaceOption = true; }
        else die(std::string("unknown option ") + key);
    }
    if (argc < 4 || volumes.empty()) {
        std::cout << "Usage : FuseLabels bbox.json spacing labels_0 ... labels_N-1 [-td transformsDir] [-o outDir] [-b background] "
                     "[-ml maxLabels] [-p 1] [-wt 1] [-dev n] [-s 1 [-sp p0] [-st tol] [-si maxIter] [-sr 0|1]] [-d 1 [-dp percentile] [-dr 0|1]]" << std::endl;
        return 1;
    }
    const size_t n = volumes.size();
    if (maxLabels < 0 || maxLabels > 65536) die("-ml : 1 to 65536 labels");
    if (n > 65535) die("at most 65535 label volumes");
    if (stapleOption && staple != 1) die("-sp, -st, -si and -sr need -s 1");
    if (staple == 1) {
        if (n > 4096) die("-s 1 takes at most 4096 label volumes");
        if (maxLabels > FROG_STAPLE_MAX_LABELS) die("-s 1 takes at most " + std::to_string(FROG_STAPLE_MAX_LABELS) + " labels (-ml)");
        if (!(stapleP0 > 0.0 && stapleP0 < 1.0)) die("-sp : a probability inside (0, 1)");
        if (!(stapleTol >= 0.0)) die("-st : a tolerance that is not negative");
        if (stapleIterations < 0 || stapleIterations > 1000000) die("-si : 0 to 1000000 iterations");
        if (stapleRestrict != 0 && stapleRestrict != 1) die("-sr : 0 or 1");
    }
    if (surfaceOption && surface != 1) die("-dp and -dr need -d 1");
    if (surface == 1) {
        if (surfacePercentile < 1 || surfacePercentile > 100) die("-dp : a percentile from 1 to 100");
        if (surfaceReference != 0 && surfaceReference != 1) die("-dr : 0 (the vote) or 1 (STAPLE)");
        if (surfaceReference == 1 && staple != 1) die("-dr 1 measures against staple.nii.gz and needs -s 1");
        // the table may hold the background beside the measured labels
        if (maxLabels > FROG_SURFACE_MAX_LABELS + 1) die("-d 1 measures at most " + std::to_string(FROG_SURFACE_MAX_LABELS) + " labels (-ml)");
    }

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
    frog_staple *em = nullptr;
    if (staple == 1 && frog_staple_create(&grid, (uint32_t)n, (uint32_t)maxLabels, device, &em)) die(frog_last_error());
    times.setup_s = seconds(t0);

    const size_t total = (size_t)grid.dims[0] * grid.dims[1] * grid.dims[2];
    ReslicedVolume resliced;
    for (size_t i = 0; i < n; i++) {
        double waited = 0;
        frog::VolumeStream::Item &it = stream.get(i, &waited);
        times.waited_s += waited;
        if (!it.file) die("cannot read volume " + volumes[i]);
        frog_volume *out = resliced.stage(writeTransformed || em, grid, it.view.dtype);
        t0 = clk::now();
        if (frog_labels_add(acc, chains[i], &it.view, background, out)) die(volumes[i] + ": " + frog_last_error());
        if (em && frog_staple_add(em, nullptr, out, background, nullptr)) die(volumes[i] + ": " + frog_last_error());
        times.device_s += seconds(t0);
        stream.release(i);
        frog_chain_destroy(chains[i]);
        chains[i] = nullptr;
        if (out && writeTransformed) {
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
    std::vector<unsigned char> vote;                        // labels.nii.gz's voxels, where STAPLE is about to take their place
    if (em && surface == 1 && surfaceReference == 0) vote = fused;
    if (em) {
        t0 = clk::now();
        uint32_t L = 0, iterations = 0;
        double change = 0;
        uint64_t active = 0;
        if (frog_staple_finish(em, &L) || frog_staple_solve(em, stapleP0, stapleTol, (uint32_t)stapleIterations, stapleRestrict, &iterations, &change, &active))
            die(frog_last_error());
        std::vector<int64_t> em_values(L);
        std::vector<double> theta((size_t)n * L * L), prior(L);
        std::vector<uint64_t> sums((size_t)n * L * L), totals(L);
        if (frog_staple_values(em, em_values.data()) || frog_staple_performance(em, theta.data(), sums.data(), totals.data(), prior.data())
            || frog_staple_fused(em, &label, share.data()))                      // the values are the vote's: the same type holds them
            die(frog_last_error());
        times.device_s += seconds(t0);

        t0 = clk::now();
        const std::string staple_path = outDir + "/staple.nii.gz", confidence_path = outDir + "/staple_confidence.nii.gz";
        if (frog_volume_write(staple_path.c_str(), &label)) die("cannot write " + staple_path);
        if (frog_volume_write(confidence_path.c_str(), &f32)) die("cannot write " + confidence_path);
        // the voxels of every label in staple.nii.gz
        std::vector<uint64_t> fused_voxels(L, 0);
        for (size_t v = 0; v < total; v++) {
            int64_t value = 0;
            switch (dtype) {
            case FROG_V_U8: value = ((const uint8_t *)fused.data())[v]; break;
            case FROG_V_U16: value = ((const uint16_t *)fused.data())[v]; break;
            case FROG_V_I16: value = ((const int16_t *)fused.data())[v]; break;
            case FROG_V_I32: value = ((const int32_t *)fused.data())[v]; break;
            default: value = ((const uint32_t *)fused.data())[v]; break;
            }
            fused_voxels[std::lower_bound(em_values.begin(), em_values.end(), value) - em_values.begin()]++;
        }
        const std::string staple_csv = outDir + "/staple.csv", performance_csv = outDir + "/performance.csv";
        csv = std::fopen(staple_csv.c_str(), "w");
        if (!csv) die("cannot write " + staple_csv);
        std::fprintf(csv, "label,prior,voxels,volume_mm3\n");
        for (uint32_t l = 0; l < L; l++)
            std::fprintf(csv, "%lld,%.17g,%llu,%.17g\n", (long long)em_values[l], prior[l], (unsigned long long)fused_voxels[l],
                         (double)fused_voxels[l] * voxel_mm3);
        if (std::fclose(csv) != 0) die("cannot write " + staple_csv);
        uint64_t all = 0;
        for (const uint64_t x : totals) all += x;
        std::vector<double> accuracy(n);
        for (size_t i = 0; i < n; i++) {
            uint64_t diagonal = 0;
            for (uint32_t l = 0; l < L; l++) diagonal += sums[(i * L + l) * L + l];
            accuracy[i] = (double)diagonal / (double)all;                       // nan where no M-step ran
        }
        std::vector<double> finite;
        for (const double x : accuracy) if (std::isfinite(x)) finite.push_back(x);
        double mid = 0, mad = 0;
        if (!finite.empty()) {
            mid = median(finite);
            for (double &x : finite) x = std::fabs(x - mid);
            mad = median(finite);
        }
        csv = std::fopen(performance_csv.c_str(), "w");
        if (!csv) die("cannot write " + performance_csv);
        std::fprintf(csv, "image,file,accuracy,accuracy_robust_z");
        for (uint32_t l = 0; l < L; l++) std::fprintf(csv, ",sensitivity_%lld", (long long)em_values[l]);
        std::fprintf(csv, "\n");
        for (size_t i = 0; i < n; i++) {
            const double z = !std::isfinite(accuracy[i]) ? NAN : (mad > 0 ? (accuracy[i] - mid) / (1.4826 * mad) : 0.0);
            std::fprintf(csv, "%zu,%s,", i, volumes[i].c_str());
            if (std::isnan(accuracy[i])) std::fprintf(csv, "nan,nan"); else std::fprintf(csv, "%.17g,%.17g", accuracy[i], z);
            for (uint32_t l = 0; l < L; l++) std::fprintf(csv, ",%.17g", theta[(i * L + l) * L + l]);
            std::fprintf(csv, "\n");
        }
        if (std::fclose(csv) != 0) die("cannot write " + performance_csv);
        times.write_s += seconds(t0);
        if (writeProbabilities) {
            for (uint32_t l = 0; l < L; l++) {
                t0 = clk::now();
                if (frog_staple_probability(em, em_values[l], share.data())) die(frog_last_error());
                times.device_s += seconds(t0);
                t0 = clk::now();
                const std::string path = outDir + "/staple_probability_" + std::to_string(em_values[l]) + ".nii.gz";
                if (frog_volume_write(path.c_str(), &f32)) die("cannot write " + path);
                times.write_s += seconds(t0);
            }
        }
        frog_staple_destroy(em);
        char line[160];
        std::snprintf(line, sizeof line, "staple : %u iterations, change %.17g, %llu active voxels", iterations, change, (unsigned long long)active);
        std::cout << line << std::endl;
    }
    // ---- -d 1: every image's surface distances to the consensus, the label maps streamed a second time
    double surface_s = 0;
    if (surface == 1) {
        t0 = clk::now();
        std::vector<int64_t> measured;
        for (const int64_t v : values) if ((double)v != background) measured.push_back(v);
        if (measured.empty()) die("-d 1 : the table holds no label besides the background");
        if (measured.size() > FROG_SURFACE_MAX_LABELS) die("-d 1 measures at most " + std::to_string(FROG_SURFACE_MAX_LABELS) + " labels");
        const size_t L = measured.size();
        label.data = vote.empty() ? fused.data() : vote.data();
        frog_surface *sd = nullptr;
        if (frog_surface_create(&label, measured.data(), (uint32_t)L, (uint32_t)surfacePercentile, device, &sd)) die(frog_last_error());
        chains = create_chains(inverse, device);
        frog::VolumeStream again(volumes, threads, window);
        std::vector<frog_surface_row> rows(n * L);
        for (size_t i = 0; i < n; i++) {
            frog::VolumeStream::Item &it = again.get(i, nullptr);
            if (!it.file) die("cannot read volume " + volumes[i]);
            if (frog_surface_add(sd, chains[i], &it.view, background, &rows[i * L])) die(volumes[i] + ": " + frog_last_error());
            again.release(i);
            frog_chain_destroy(chains[i]);
            chains[i] = nullptr;
        }
        frog_surface_destroy(sd);

        const std::string p = std::to_string(surfacePercentile);
        const std::string rows_csv = outDir + "/surface.csv", images_csv = outDir + "/surface_images.csv", labels_csv = outDir + "/surface_labels.csv";
        csv = std::fopen(rows_csv.c_str(), "w");
        if (!csv) die("cannot write " + rows_csv);
        std::fprintf(csv, "image,file,label,surface_voxels,reference_surface_voxels,hausdorff,hausdorff_%s,assd\n", p.c_str());
        std::vector<SurfaceMetrics> metrics(n * L);
        for (size_t i = 0; i < n; i++) {
            for (size_t l = 0; l < L; l++) {
                const frog_surface_row &r = rows[i * L + l];
                const SurfaceMetrics &m = metrics[i * L + l] = surface_metrics(r);
                std::fprintf(csv, "%zu,%s,%lld,%llu,%llu,%s,%s,%s\n", i, volumes[i].c_str(), (long long)measured[l], (unsigned long long)r.n_a,
                             (unsigned long long)r.n_b, g17(m.hausdorff).c_str(), g17(m.hausdorff_p).c_str(), g17(m.assd).c_str());
            }
        }
        if (std::fclose(csv) != 0) die("cannot write " + rows_csv);

        std::vector<double> mean_assd(n), largest(n);
        std::vector<size_t> labels_measured(n);
        for (size_t i = 0; i < n; i++) {
            std::vector<double> assd;
            largest[i] = NAN;
            for (size_t l = 0; l < L; l++) {
                const SurfaceMetrics &m = metrics[i * L + l];
                if (std::isnan(m.assd)) continue;
                assd.push_back(m.assd);
                if (std::isnan(largest[i]) || m.hausdorff > largest[i]) largest[i] = m.hausdorff;
            }
            labels_measured[i] = assd.size();
            mean_assd[i] = mean_in_order(assd);
        }
        std::vector<double> finite;
        for (const double x : mean_assd) if (std::isfinite(x)) finite.push_back(x);
        double mid = 0, mad = 0;
        if (!finite.empty()) {
            mid = median(finite);
            for (double &x : finite) x = std::fabs(x - mid);
            mad = median(finite);
        }
        csv = std::fopen(images_csv.c_str(), "w");
        if (!csv) die("cannot write " + images_csv);
        std::fprintf(csv, "image,file,labels_measured,mean_assd,mean_assd_robust_z,max_hausdorff\n");
        for (size_t i = 0; i < n; i++) {
            const double z = !std::isfinite(mean_assd[i]) ? NAN : (mad > 0 ? (mean_assd[i] - mid) / (1.4826 * mad) : 0.0);
            std::fprintf(csv, "%zu,%s,%zu,%s,%s,%s\n", i, volumes[i].c_str(), labels_measured[i], g17(mean_assd[i]).c_str(), g17(z).c_str(),
                         g17(largest[i]).c_str());
        }
        if (std::fclose(csv) != 0) die("cannot write " + images_csv);

        csv = std::fopen(labels_csv.c_str(), "w");
        if (!csv) die("cannot write " + labels_csv);
        std::fprintf(csv, "label,images_measured,mean_assd,max_hausdorff,mean_hausdorff_%s\n", p.c_str());
        for (size_t l = 0; l < L; l++) {
            std::vector<double> assd, hausdorff_p;
            double top = NAN;
            for (size_t i = 0; i < n; i++) {
                const SurfaceMetrics &m = metrics[i * L + l];
                if (std::isnan(m.assd)) continue;
                assd.push_back(m.assd);
                hausdorff_p.push_back(m.hausdorff_p);
                if (std::isnan(top) || m.hausdorff > top) top = m.hausdorff;
            }
            std::fprintf(csv, "%lld,%zu,%s,%s,%s\n", (long long)measured[l], assd.size(), g17(mean_in_order(assd)).c_str(), g17(top).c_str(),
                         g17(mean_in_order(hausdorff_p)).c_str());
        }
        if (std::fclose(csv) != 0) die("cannot write " + labels_csv);
        surface_s = seconds(t0);
    }
    times.print(stream.read_seconds(), stream.threads());
    if (surface == 1) {
        char line[64];
        std::snprintf(line, sizeof line, "surface : %.3f s", surface_s);
        std::cout << line << std::endl;
    }
    return 0;
}
