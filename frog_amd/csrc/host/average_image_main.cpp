// AverageImage: the group's average and stdev images in one process -- what transform.sh (and FROG.py -a) computes with
// DummyVolumeGenerator, one VolumeTransform per image and AverageVolumes, without writing and re-reading N volumes and
// without N + 2 HIP runtime starts.
//   AverageImage bbox.json spacing v_0 ... v_{N-1} [-td transformsDir] [-o outDir] [-i interpolation] [-b background]
//                [-wt 1] [-dev n] [-c 1 [-ml masks.txt] [-mc minCount] [-f fill]] [-q 1 [-qb bins] [-qr lo hi]]
//                [-r 1 [-rq q1,q2,...] [-rp planes]]
// The grid is DummyVolumeGenerator's (frog_bbox_grid); image i is resliced through the inverse of <transformsDir>/<i>.json
// (default "transforms"; -j and sidecar forms) exactly as `VolumeTransform v_i dummy.mhd -t transforms/i.json` does it
// (same device code; background = the image's minimum unless -b, linear unless -i 0), converted to its own type and added
// on the device (frog_average_add) in image order, so average.nii.gz and stdev.nii.gz in outDir are AverageVolumes' files
// bit for bit.  -wt 1 also writes transformed<i>.nii.gz, the file transform.sh leaves behind.  Every transform and volume
// header is checked before anything is written.  Volumes are read and inflated on host threads ahead of the device, a
// bounded number at a time (volume_stream.h).
// -c 1 (coverage-aware; no counterpart upstream): image i is added only where it covers the grid voxel (frog_cover_add), so
// average.nii.gz and stdev.nii.gz are the mean and the population stdev over the covering images, and coverage.nii.gz
// (uint16) is their number.  -ml names a text file with one mask path per line, N lines (the list format of FROG.py -m):
// image i then counts only where mask i, an integer volume of its own geometry, is non-zero at the nearest voxel; the masks
// are streamed like the images.  -mc: voxels that fewer than minCount (default 1) images cover get the mean -f (default 0)
// and the stdev 0.  -ml, -mc or -f without -c 1 is an error.  transformed<i>.nii.gz is the same file either way.
// -q 1 (with -c 1; which images registered badly?): after the average is written the images and masks are streamed a second
// time, in the same order, and each is scored against the mean of the OTHER images over the voxels it covers and at least
// max(2, minCount) images do (frog_cover_score with leave_one_out, frog_score_metrics_from).  quality.csv in outDir has one
// row per image: image,file,voxels,covered_fraction,ncc,nmi,mi,mean_abs_diff,rmse,ncc_robust_z -- voxels = the voxels that
// entered the sums, covered_fraction = voxels / grid voxels, ncc_robust_z = (ncc - median) / (1.4826 MAD) over the group's
// finite nccs (0 where the MAD is 0; the median of an even number is the mean of the middle two); doubles as %.17g, NaN as
// nan.  -qb: bins per axis of the joint histogram behind mi and nmi (2..64, default 64).  -qr lo hi: its value range, by
// default the smallest finite value of the mean over the voxels that minCount images cover and the float after the largest;
// the range used is printed.  The average's files and the first pass are the same with and without -q 1.
// -r 1 (with -c 1; the robust atlas): after the average is written, and after the -q 1 pass if there is one, the images and
// masks are streamed again, once per slab of z-planes, and every image's value is kept per voxel (frog_rank_add) under the
// validity rule of -c 1; median.nii.gz and mad.nii.gz (FLOAT32) are then the per-voxel median and the raw median absolute
// deviation (x 1.4826 for a normal stdev) over the covering images whose value is not NaN.  -rq: up to 15 probabilities in
// [0, 1], comma-separated; each gives quantile_<text as typed>.nii.gz (linear interpolation between the neighbouring order
// statistics).  -mc and -f apply as they do to the mean (the MAD is 0 where the mean is the fill).  A slab is as many planes
// as frog_rank_planes allows (half of the free device memory at 4 bytes per image and voxel), or -rp planes if that is
// fewer; the slab count is printed and changes no bit of the files.  -rq or -rp without -r 1 is an error; every other file
// is the same with and without -r 1.
#include "group_tool.h"
#include "volume_stream.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

namespace {

// the median of a non-empty list: the middle value, or the mean of the middle two
double median(std::vector<double> v)
{
    std::sort(v.begin(), v.end());
    const size_t n = v.size();
    return n % 2 ? v[n / 2] : (v[n / 2 - 1] + v[n / 2]) / 2.0;
}

// %.17g, which reads back to the same double; a NaN of either sign as "nan"
std::string csv_double(double v)
{
    if (std::isnan(v)) return "nan";
    char buf[40];
    std::snprintf(buf, sizeof buf, "%.17g", v);
    return buf;
}

// -rq's list: up to 15 comma-separated probabilities in [0, 1], each kept as typed for its file name
void parse_quantiles(const std::string &list, std::vector<std::string> &texts, std::vector<double> &values)
{
    for (size_t at = 0; at <= list.size();) {
        const size_t comma = std::min(list.find(',', at), list.size());
        const std::string text = list.substr(at, comma - at);
        char *end = nullptr;
        const double q = std::strtod(text.c_str(), &end);
        if (text.empty() || *end || !(q >= 0.0 && q <= 1.0))
            die("-rq takes comma-separated probabilities in [0, 1], not '" + text + "'");
        texts.push_back(text);
        values.push_back(q);
        at = comma + 1;
    }
    if (values.size() > 15) die("-rq takes at most 15 probabilities");
}

} // namespace

int main(int argc, char *argv[])
{
    PhaseTimes times;
    std::vector<std::string> volumes;
    std::string transformsDir = "transforms", outDir = ".", maskList;
    int interpolation = 1, device = 0, writeTransformed = 0, coverage = 0, quality = 0, robust = 0;
    long minCount = 1, qualityBins = 64, robustPlanes = 0;
    float fill = 0, qualityLo = 0, qualityHi = 0;
    bool qualityOption = false, qualityRange = false;       // -qb or -qr was given; -qr was given
    bool coverageOption = false;                            // -ml, -mc or -f was given
    bool robustListOption = false, robustPlanesOption = false;  // -rq was given; -rp was given
    std::string robustList;
    BackgroundLevel background;
    int a = positional_arguments(argc, argv, 3, { "-td", "-o", "-i", "-b", "-wt", "-dev", "-c", "-ml", "-mc", "-f", "-q", "-qb", "-qr", "-r", "-rq", "-rp" }, volumes);
    for (; a < argc; a += 2) {
        const char *key = argv[a], *value = a + 1 < argc ? argv[a + 1] : "";
        if (std::strcmp(key, "-td") == 0) transformsDir = value;
        else if (std::strcmp(key, "-o") == 0) outDir = value;
        else if (std::strcmp(key, "-i") == 0) interpolation = atoi(value);
        else if (std::strcmp(key, "-b") == 0) background.parse(value);
        else if (std::strcmp(key, "-wt") == 0) writeTransformed = atoi(value);
        else if (std::strcmp(key, "-dev") == 0) device = atoi(value);
        else if (std::strcmp(key, "-c") == 0) coverage = atoi(value);
        else if (std::strcmp(key, "-ml") == 0) { maskList = value; coverageOption = true; }
        else if (std::strcmp(key, "-mc") == 0) { minCount = atol(value); coverageOption = true; }
        else if (std::strcmp(key, "-f") == 0) { fill = (float)atof(value); coverageOption = true; }
        else if (std::strcmp(key, "-q") == 0) quality = atoi(value);
        else if (std::strcmp(key, "-qb") == 0) { qualityBins = atol(value); qualityOption = true; }
        else if (std::strcmp(key, "-qr") == 0) {            // two values
            qualityLo = (float)atof(value);
            qualityHi = (float)atof(a + 2 < argc ? argv[a + 2] : "");
            qualityOption = qualityRange = true;
            a++;
        }
        else if (std::strcmp(key, "-r") == 0) robust = atoi(value);
        else if (std::strcmp(key, "-rq") == 0) { robustList = value; robustListOption = true; }
        else if (std::strcmp(key, "-rp") == 0) { robustPlanes = atol(value); robustPlanesOption = true; }
        else die(std::string("unknown option ") + key);
    }
    if (argc < 4 || volumes.empty()) {
        std::cout << "Usage : AverageImage bbox.json spacing image_0 ... image_N-1 [-td transformsDir] [-o outDir] [-i interpolation] "
                     "[-b background] [-wt 1] [-dev n] [-c 1 [-ml masks.txt] [-mc minCount] [-f fill]] [-q 1 [-qb bins] [-qr lo hi]] "
                     "[-r 1 [-rq q1,q2,...] [-rp planes]]" << std::endl;
        return 1;
    }
    const size_t n = volumes.size();
    if (coverageOption && coverage != 1) die("-ml, -mc and -f need -c 1");
    if (minCount < 1 || minCount > 65535) die("-mc takes a count from 1 to 65535");
    if (quality == 1 && coverage != 1) die("-q 1 scores the images against the coverage-aware average: it needs -c 1");
    if (qualityOption && quality != 1) die("-qb and -qr need -q 1");
    if (qualityBins < 2 || qualityBins > 64) die("-qb takes 2 to 64 bins");
    if (qualityRange && !(std::isfinite(qualityLo) && std::isfinite(qualityHi) && qualityHi > qualityLo && std::isfinite(qualityHi - qualityLo)))
        die("-qr takes two finite values lo < hi");
    if (robust == 1 && coverage != 1) die("-r 1 ranks the images under the coverage rule: it needs -c 1");
    if ((robustListOption || robustPlanesOption) && robust != 1) die("-rq and -rp need -r 1");
    if (robustPlanesOption && robustPlanes < 1) die("-rp takes a number of planes, at least 1");
    if (robust == 1 && n > FROG_RANK_MAX_IMAGES) die("-r 1 takes at most " + std::to_string(FROG_RANK_MAX_IMAGES) + " images");
    std::vector<std::string> quantileTexts;
    std::vector<double> probabilities{ 0.5 };               // the median first, then -rq's
    if (robustListOption) parse_quantiles(robustList, quantileTexts, probabilities);
    if (coverage == 1 && n > 65535) die("-c 1 takes at most 65535 images (16-bit counts)");
    std::vector<std::string> masks;
    if (!maskList.empty()) {
        if (!read_list(maskList, masks)) die("cannot read the mask list " + maskList);
        if (masks.size() != n) die(maskList + " holds " + std::to_string(masks.size()) + " masks for " + std::to_string(n) + " images");
    }

    // ---- everything is checked before the first output: the grid, every transform, every volume header
    frog_volume grid;
    if (frog_bbox_grid(argv[1], atof(argv[2]), &grid)) die(std::string("cannot read a bounding box from ") + argv[1] + " (or spacing " + argv[2] + " is not positive)");
    ChainArguments transforms;
    const auto inverse = inverse_transforms(transforms, transformsDir, n);
    for (const auto &v : volumes) if (!peek_header(v).ok) die("cannot read volume " + v);
    for (const auto &m : masks) {
        const VolumeHeader h = peek_header(m);
        if (!h.ok) die("cannot read mask " + m);
        if (h.is_float) die(m + " is a float volume: masks have an integer type");
    }
    begin_output(outDir, n, "images", grid);

    int threads;
    size_t window;
    frog::volume_stream_shape(n, &threads, &window);
    if (!masks.empty()) threads = std::max(1, threads / 2);  // the masks have readers of their own
    frog::VolumeStream stream(volumes, threads, window);     // reading starts now, beside the device set-up below
    std::unique_ptr<frog::VolumeStream> maskStream(masks.empty() ? nullptr : new frog::VolumeStream(masks, threads, window));

    auto t0 = clk::now();
    std::vector<frog_chain *> chains = create_chains(inverse, device);
    frog_average *avg = nullptr;
    frog_cover *cover = nullptr;
    if (coverage == 1 ? frog_cover_create(&grid, device, &cover) : frog_average_create(&grid, (uint32_t)n, device, &avg)) die(frog_last_error());
    times.setup_s = seconds(t0);

    const size_t total = (size_t)grid.dims[0] * grid.dims[1] * grid.dims[2];
    ReslicedVolume resliced;
    for (size_t i = 0; i < n; i++) {
        double waited = 0;
        frog::VolumeStream::Item &it = stream.get(i, &waited);
        times.waited_s += waited;
        if (!it.file) die("cannot read volume " + volumes[i]);
        const frog_volume *mask = nullptr;
        if (maskStream) {
            frog::VolumeStream::Item &m = maskStream->get(i, &waited);
            times.waited_s += waited;
            if (!m.file) die("cannot read mask " + masks[i]);
            mask = &m.view;
        }
        frog_volume *out = resliced.stage(writeTransformed, grid, it.view.dtype);
        t0 = clk::now();
        if (cover ? frog_cover_add(cover, chains[i], &it.view, mask, interpolation, background.of(it.lo), out)
                  : frog_average_add(avg, chains[i], &it.view, interpolation, background.of(it.lo), out))
            die(volumes[i] + ": " + frog_last_error());
        times.device_s += seconds(t0);
        stream.release(i);
        if (maskStream) maskStream->release(i);
        if (quality != 1 && robust != 1) {                  // a later pass evaluates the chain again
            frog_chain_destroy(chains[i]);
            chains[i] = nullptr;
        }
        if (out) {
            t0 = clk::now();
            resliced.write(outDir, "transformed", i);
            times.write_s += seconds(t0);
        }
    }
    std::vector<float> mean(total), stdev(total);
    std::vector<uint16_t> count(cover ? total : 0);
    t0 = clk::now();
    if (cover ? frog_cover_finish(cover, (uint32_t)minCount, fill, mean.data(), stdev.data(), count.data())
              : frog_average_finish(avg, mean.data(), stdev.data())) die(frog_last_error());
    times.device_s += seconds(t0);
    frog_average_destroy(avg);

    t0 = clk::now();
    grid.dtype = FROG_V_F32;
    for (auto [name, data] : { std::make_pair("average.nii.gz", mean.data()), std::make_pair("stdev.nii.gz", stdev.data()) }) {
        grid.data = data;
        const std::string path = outDir + "/" + name;
        if (frog_volume_write(path.c_str(), &grid)) die("cannot write " + path);
    }
    if (cover) {
        grid.dtype = FROG_V_U16;
        grid.data = count.data();
        const std::string path = outDir + "/coverage.nii.gz";
        if (frog_volume_write(path.c_str(), &grid)) die("cannot write " + path);
    }
    times.write_s += seconds(t0);

    // ---- -q 1: every image against the mean of the others, the files streamed once more in the same order
    double quality_s = 0;
    if (quality == 1) {
        t0 = clk::now();
        if (!qualityRange) {
            bool any = false;
            for (size_t v = 0; v < total; v++) {
                if (count[v] < minCount || !std::isfinite(mean[v])) continue;
                if (!any || mean[v] < qualityLo) qualityLo = mean[v];
                if (!any || mean[v] > qualityHi) qualityHi = mean[v];
                any = true;
            }
            if (!any) die("-q 1: no voxel with a finite mean that " + std::to_string(minCount) + " images cover");
            qualityHi = std::nextafterf(qualityHi, INFINITY);
        }
        std::cout << "quality : " << qualityBins << " x " << qualityBins << " bins over [" << csv_double(qualityLo) << ", " << csv_double(qualityHi) << ")" << std::endl;
        frog::VolumeStream again(volumes, threads, window);
        std::unique_ptr<frog::VolumeStream> maskAgain(masks.empty() ? nullptr : new frog::VolumeStream(masks, threads, window));
        std::vector<frog_score_sums> sums(n);
        std::vector<frog_score_metrics> metrics(n);
        std::vector<uint64_t> histogram((size_t)qualityBins * qualityBins);
        for (size_t i = 0; i < n; i++) {
            frog::VolumeStream::Item &it = again.get(i, nullptr);
            if (!it.file) die("cannot read volume " + volumes[i]);
            const frog_volume *mask = nullptr;
            if (maskAgain) {
                frog::VolumeStream::Item &m = maskAgain->get(i, nullptr);
                if (!m.file) die("cannot read mask " + masks[i]);
                mask = &m.view;
            }
            if (frog_cover_score(cover, chains[i], &it.view, mask, interpolation, background.of(it.lo), (uint32_t)minCount, 1,
                                 (uint32_t)qualityBins, qualityLo, qualityHi, &sums[i], histogram.data())
                || frog_score_metrics_from(&sums[i], histogram.data(), (uint32_t)qualityBins, &metrics[i]))
                die(volumes[i] + ": " + frog_last_error());
            again.release(i);
            if (maskAgain) maskAgain->release(i);
            if (robust != 1) {
                frog_chain_destroy(chains[i]);
                chains[i] = nullptr;
            }
        }
        std::vector<double> finite;
        for (const auto &m : metrics) if (std::isfinite(m.ncc)) finite.push_back(m.ncc);
        double mid = 0, mad = 0;
        if (!finite.empty()) {
            mid = median(finite);
            for (double &v : finite) v = std::fabs(v - mid);
            mad = median(finite);
        }
        const std::string path = outDir + "/quality.csv";
        std::ofstream csv(path);
        csv << "image,file,voxels,covered_fraction,ncc,nmi,mi,mean_abs_diff,rmse,ncc_robust_z\n";
        for (size_t i = 0; i < n; i++) {
            const frog_score_metrics &m = metrics[i];
            const double z = !std::isfinite(m.ncc) ? NAN : (mad > 0 ? (m.ncc - mid) / (1.4826 * mad) : 0.0);
            csv << i << "," << volumes[i] << "," << sums[i].n << "," << csv_double((double)sums[i].n / (double)total) << "," << csv_double(m.ncc)
                << "," << csv_double(m.nmi) << "," << csv_double(m.mi) << "," << csv_double(m.mean_abs_diff) << "," << csv_double(m.rmse)
                << "," << csv_double(z) << "\n";
        }
        csv.close();
        if (!csv) die("cannot write " + path);
        quality_s = seconds(t0);
    }
    frog_cover_destroy(cover);

    // ---- -r 1: median, MAD and quantile images, the files streamed once more per slab of z-planes
    double robust_s = 0;
    if (robust == 1) {
        t0 = clk::now();
        uint32_t planes = 0;
        if (frog_rank_planes(&grid, (uint32_t)n, device, &planes)) die(frog_last_error());
        if (robustPlanesOption && (uint64_t)robustPlanes < planes) planes = (uint32_t)robustPlanes;
        const uint32_t depth = grid.dims[2], slabs = (depth + planes - 1) / planes;
        std::cout << "robust : " << slabs << (slabs == 1 ? " slab of " : " slabs of ") << planes << " planes, " << probabilities.size()
                  << " probabilities" << std::endl;
        const size_t n_q = probabilities.size(), plane = (size_t)grid.dims[0] * grid.dims[1];
        std::vector<float> values(n_q * total), mad(total), slabValues;
        for (uint32_t first = 0; first < depth; first += planes) {
            const uint32_t count_planes = std::min(planes, depth - first);
            const size_t slabVoxels = plane * count_planes;
            frog_rank *rank = nullptr;
            if (frog_rank_create(&grid, first, count_planes, (uint32_t)n, device, &rank)) die(frog_last_error());
            frog::VolumeStream again(volumes, threads, window);
            std::unique_ptr<frog::VolumeStream> maskAgain(masks.empty() ? nullptr : new frog::VolumeStream(masks, threads, window));
            const bool last = first + count_planes >= depth;
            for (size_t i = 0; i < n; i++) {
                frog::VolumeStream::Item &it = again.get(i, nullptr);
                if (!it.file) die("cannot read volume " + volumes[i]);
                const frog_volume *mask = nullptr;
                if (maskAgain) {
                    frog::VolumeStream::Item &m = maskAgain->get(i, nullptr);
                    if (!m.file) die("cannot read mask " + masks[i]);
                    mask = &m.view;
                }
                if (frog_rank_add(rank, chains[i], &it.view, mask, interpolation, background.of(it.lo))) die(volumes[i] + ": " + frog_last_error());
                again.release(i);
                if (maskAgain) maskAgain->release(i);
                if (last) {
                    frog_chain_destroy(chains[i]);
                    chains[i] = nullptr;
                }
            }
            slabValues.resize(n_q * slabVoxels);
            if (frog_rank_finish(rank, (uint32_t)minCount, fill, (uint32_t)n_q, probabilities.data(), slabValues.data(),
                                 mad.data() + plane * first, nullptr)) die(frog_last_error());
            for (size_t j = 0; j < n_q; j++)
                std::memcpy(values.data() + j * total + plane * first, slabValues.data() + j * slabVoxels, slabVoxels * sizeof(float));
            frog_rank_destroy(rank);
        }
        grid.dtype = FROG_V_F32;
        auto write = [&](const std::string &name, float *data) {
            grid.data = data;
            const std::string path = outDir + "/" + name;
            if (frog_volume_write(path.c_str(), &grid)) die("cannot write " + path);
        };
        write("median.nii.gz", values.data());
        write("mad.nii.gz", mad.data());
        for (size_t j = 1; j < n_q; j++) write("quantile_" + quantileTexts[j - 1] + ".nii.gz", values.data() + j * total);
        robust_s = seconds(t0);
    }
    times.print(stream.read_seconds() + (maskStream ? maskStream->read_seconds() : 0.0), stream.threads() + (maskStream ? maskStream->threads() : 0));
    if (quality == 1) {
        char line[64];
        std::snprintf(line, sizeof line, "quality : %.3f s", quality_s);
        std::cout << line << std::endl;
    }
    if (robust == 1) {
        char line[64];
        std::snprintf(line, sizeof line, "robust : %.3f s", robust_s);
        std::cout << line << std::endl;
    }
    return 0;
}
