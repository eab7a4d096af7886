// GroupStats: where do the images of a registered group differ from each other -- a per-voxel linear model of the images'
// values on a design matrix, one t-map per contrast, and a permutation test of the maximum statistic for p-values corrected
// over all voxels (frog_glm, include/frog_chain.h, which states the arithmetic).
//   GroupStats bbox.json spacing design.csv [-c contrasts.csv] [-td transformsDir] [-o outDir] [-v jacobian|logjacobian|images]
//              [-vl volumes.txt] [-ml masks.txt] [-m regionMask] [-mc minCount] [-sf sigmaFloor] [-f fill] [-np nPerms]
//              [-ps seed] [-pc columns] [-pf 1] [-two 1] [-ct threshold] [-cc 6|18|26] [-tf 1] [-tfd dh] [-tfe 0.5|1] [-tfh 1|2]
//              [-s fwhm_mm] [-rp planes] [-dev n]
// The grid is DummyVolumeGenerator's (frog_bbox_grid).  design.csv has one row per image and one column per regressor,
// numbers separated by commas or blanks, after an optional header line; row i belongs to <transformsDir>/<i>.json (default
// "transforms"), which is inverted as AverageImage inverts it.  -c: one contrast per row, as many numbers as the design has
// columns; by default one unit contrast per column that is not constant.
// -v (default logjacobian): the value of image i at a grid voxel.  logjacobian and jacobian need no image data: the
// determinant of the chain's Jacobian there (what TransformField writes), or its logarithm where it is positive; with -vl, a
// list of N volume paths, the voxel counts only where the chain lands inside volume i's geometry (its header alone is read).
// images: the volumes of -vl resliced and counted as AverageImage -c 1 does (linear interpolation).  -ml: N mask paths, as in
// AverageImage.  -m: an integer volume on the grid; the model is fit only where it is non-zero.  -mc: fewer participating
// images than minCount (and always than columns + 1) leave a voxel unfit; unfit voxels hold -f (default 0).  -sf: a residual
// stdev at or below sigmaFloor (default 0) gives t = NaN.
// Outputs in outDir: beta_<j>.nii.gz, sigma.nii.gz, t_<c>.nii.gz (FLOAT32), count.nii.gz (UINT16), glm.csv with one row per
// contrast: contrast, fit_voxels (fit and t not NaN), peak_t, peak_x, peak_y, peak_z, threshold_p05, voxels_p05.
// -np nPerms: permutation 0 is the design itself, the others move the rows of the columns -pc (comma-separated indices; by
// default the columns with a non-zero entry in any contrast) by frog_glm_draw(seed -ps, default 0); -pf 1 also flips signs.
// fwe_p_<c>.nii.gz = (float)((1 + #{k >= 1 : max_t[k][c] >= t}) / (double)nPerms), 1 where the voxel is unfit or t is NaN;
// -two 1 compares |t| with max(max_t, -min_t).  maxt.csv: permutation,contrast,max,min as %.9g.  threshold_p05 is the largest
// null maximum a t must exceed for p < 0.05 (inf where no count of exceedances gives that), voxels_p05 the voxels that do.
// -ct threshold (needs -np): the cluster-extent test (frog_clusters).  The voxels with t > threshold, and with -two 1 also
// those with t < -threshold, form clusters at connectivity -cc (default 26: faces, edges and corners; needs -ct or -tf); a cluster's
// p is (float)((1 + #{k >= 1 : extent[k][c] >= its voxels}) / (double)nPerms), extent[k][c] the largest cluster under
// permutation k, with -two 1 the larger of the two sides'.  clusters_<c>.nii.gz (INT32): the observed map's clusters 1..K in
// ascending order of their smallest voxel index, the negative side's after the positive side's.  cluster_p_<c>.nii.gz
// (FLOAT32): the p of the voxel's cluster, 1 elsewhere.  clusters.csv: contrast,cluster,sign,voxels,peak_t,peak_x,peak_y,
// peak_z,p_fwe, the peak the largest |t| of the cluster, the smallest index among equals.  maxextent.csv:
// permutation,contrast,extent.  One sink on the device holds every permutation's masks for the whole grid, so a cluster that
// crosses slabs is one cluster; if it does not fit, the tool says how many bytes it needs and stops before the first output.
// -tf 1 (needs -np): threshold-free cluster enhancement (frog_tfce), which needs no cluster-forming threshold.  A voxel's t
// becomes the sum, over the levels k * dh (-tfd, default 0.1) up to its own, of extent^E * height^H * dh, extent the voxels of
// its cluster at that level at connectivity -cc, E = -tfe (0.5 or 1, default 0.5), H = -tfh (1 or 2, default 2); a t beyond
// 255 * dh counts as 255 * dh.  tfce_<c>.nii.gz (FLOAT32): the observed enhanced map, with -two 1 the negative side's values
// negated.  tfce_p_<c>.nii.gz = (float)((1 + #{k >= 1 : max_tfce[k][c] >= |tfce|}) / (double)nPerms), 1 where tfce is 0,
// max_tfce[k][c] the largest enhanced value under permutation k, with -two 1 the larger of the two sides'.  maxtfce.csv:
// permutation,contrast,max_tfce.  tfce.csv: contrast,peak_tfce,peak_x,peak_y,peak_z,threshold_p05,voxels_p05, as in glm.csv.
// One sink on the device holds every permutation's levels for the whole grid, one byte per voxel; if it does not fit, the tool
// says how many bytes it needs and stops before the first output.  -tf and -ct may be given together.
// -s fwhm_mm: every image's map is smoothed before the fit by the coverage-aware Gaussian of frog_glm_smooth, sigma = fwhm /
// 2.3548200450309493 (FROG_SMOOTH_FWHM): a normalised convolution over the voxels at which the image takes part, so count.nii.gz
// does not change and no background enters an image's rim.  A radius (3 sigma, in voxels) above 64 is refused.  -s 0, the
// default, changes no byte of any file.  The slabs are then those of frog_glm_smooth_planes, which leave room for the scratch
// of a slab's halo, and the line "stats :" names the FWHM, sigma and the three radii.
// The device holds slabs of frog_glm_planes z-planes, or -rp planes if that is fewer; the slab count is printed and changes no
// bit of any file.  Every input is checked before anything is written.
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

// The numeric rows of a CSV: fields separated by commas, semicolons or blanks.  A first line with a field that is not a
// number is a header and is dropped; any later one is an error.  Every row has the first row's length.
std::vector<std::vector<double>> read_table(const std::string &path, const char *what)
{
    std::vector<std::string> lines;
    if (!read_list(path, lines)) die(std::string("cannot read ") + what + " " + path);
    std::vector<std::vector<double>> rows;
    for (size_t l = 0; l < lines.size(); l++) {
        std::vector<double> row;
        bool numeric = true;
        for (size_t at = 0; at < lines[l].size();) {
            const size_t end = std::min(lines[l].find_first_of(",; \t", at), lines[l].size());
            if (end > at) {
                const std::string field = lines[l].substr(at, end - at);
                char *stop = nullptr;
                const double v = std::strtod(field.c_str(), &stop);
                if (*stop) numeric = false;
                row.push_back(v);
            }
            at = end + 1;
        }
        if (!numeric && l == 0) continue;
        if (!numeric) die(path + ": line " + std::to_string(l + 1) + " is not numeric");
        if (row.empty()) continue;
        if (!rows.empty() && row.size() != rows[0].size()) die(path + ": line " + std::to_string(l + 1) + " has another number of fields");
        for (const double v : row) if (!std::isfinite(v)) die(path + ": line " + std::to_string(l + 1) + " holds a value that is not finite");
        rows.push_back(row);
    }
    if (rows.empty()) die(path + " holds no rows");
    return rows;
}

// frog_rank's key of a float: unsigned order is the order of the floats, -0 < +0
uint32_t float_key(float x)
{
    uint32_t u;
    std::memcpy(&u, &x, sizeof u);
    return (u & 0x80000000u) ? ~u : (u ^ 0x80000000u);
}

std::string csv_float(float v)
{
    if (std::isnan(v)) return "nan";
    char buf[40];
    std::snprintf(buf, sizeof buf, "%.9g", (double)v);
    return buf;
}

} // namespace

int main(int argc, char *argv[])
{
    PhaseTimes times;
    std::vector<std::string> positional;
    std::string transformsDir = "transforms", outDir = ".", contrastsPath, valueName = "logjacobian", volumeList, maskList, regionPath, columnList;
    int device = 0, flips = 0, twoSided = 0, connectivity = 26;
    long minCount = 1, nPerms = 0, planesOption = 0;
    unsigned long long seed = 0;
    double sigmaFloor = 0, clusterThreshold = 0, tfceStep = 0.1, tfceE = 0.5, tfceH = 2, fwhm = 0;
    std::string fwhmText = "0";
    float fill = 0;
    bool planesGiven = false, permOption = false, clusterTest = false, connectivityGiven = false, tfceOption = false;
    int tfceTest = 0;
    int a = positional_arguments(argc, argv, 1, { "-c", "-td", "-o", "-v", "-vl", "-ml", "-m", "-mc", "-sf", "-f", "-np", "-ps", "-pc", "-pf", "-two", "-ct", "-cc", "-tf", "-tfd", "-tfe", "-tfh", "-s", "-rp", "-dev" },
                                 positional);
    for (; a < argc; a += 2) {
        const char *key = argv[a], *value = a + 1 < argc ? argv[a + 1] : "";
        if (std::strcmp(key, "-c") == 0) contrastsPath = value;
        else if (std::strcmp(key, "-td") == 0) transformsDir = value;
        else if (std::strcmp(key, "-o") == 0) outDir = value;
        else if (std::strcmp(key, "-v") == 0) valueName = value;
        else if (std::strcmp(key, "-vl") == 0) volumeList = value;
        else if (std::strcmp(key, "-ml") == 0) maskList = value;
        else if (std::strcmp(key, "-m") == 0) regionPath = value;
        else if (std::strcmp(key, "-mc") == 0) minCount = atol(value);
        else if (std::strcmp(key, "-sf") == 0) sigmaFloor = atof(value);
        else if (std::strcmp(key, "-f") == 0) fill = (float)atof(value);
        else if (std::strcmp(key, "-np") == 0) nPerms = atol(value);
        else if (std::strcmp(key, "-ps") == 0) { seed = std::strtoull(value, nullptr, 10); permOption = true; }
        else if (std::strcmp(key, "-pc") == 0) { columnList = value; permOption = true; }
        else if (std::strcmp(key, "-pf") == 0) { flips = atoi(value); permOption = true; }
        else if (std::strcmp(key, "-two") == 0) { twoSided = atoi(value); permOption = true; }
        else if (std::strcmp(key, "-ct") == 0) { clusterThreshold = atof(value); clusterTest = true; }
        else if (std::strcmp(key, "-cc") == 0) { connectivity = atoi(value); connectivityGiven = true; }
        else if (std::strcmp(key, "-tf") == 0) tfceTest = atoi(value);
        else if (std::strcmp(key, "-tfd") == 0) { tfceStep = atof(value); tfceOption = true; }
        else if (std::strcmp(key, "-tfe") == 0) { tfceE = atof(value); tfceOption = true; }
        else if (std::strcmp(key, "-tfh") == 0) { tfceH = atof(value); tfceOption = true; }
        else if (std::strcmp(key, "-s") == 0) fwhmText = value;
        else if (std::strcmp(key, "-rp") == 0) { planesOption = atol(value); planesGiven = true; }
        else if (std::strcmp(key, "-dev") == 0) device = atoi(value);
        else die(std::string("unknown option ") + key);
    }
    if (positional.size() != 3) {
        std::cout << "Usage : GroupStats bbox.json spacing design.csv [-c contrasts.csv] [-td transformsDir] [-o outDir] "
                     "[-v jacobian|logjacobian|images] [-vl volumes.txt] [-ml masks.txt] [-m regionMask] [-mc minCount] [-sf sigmaFloor] "
                     "[-f fill] [-np nPerms] [-ps seed] [-pc columns] [-pf 1] [-two 1] [-ct threshold] [-cc 6|18|26] [-tf 1] [-tfd dh] [-tfe 0.5|1] [-tfh 1|2] "
                     "[-s fwhm_mm] [-rp planes] [-dev n]\n-tf 1: threshold-free cluster enhancement in steps of dh (default 0.1); a statistic beyond 255 * dh "
                     "saturates there" << std::endl;
        return 1;
    }

    // ---- everything is checked before the first output
    const bool images = valueName == "images", logMode = valueName == "logjacobian";
    if (!images && !logMode && valueName != "jacobian") die("-v takes jacobian, logjacobian or images, not '" + valueName + "'");
    if (images && volumeList.empty()) die("-v images needs the volumes: -vl volumes.txt");
    if (minCount < 1 || minCount > 65535) die("-mc takes a count from 1 to 65535");
    if (!(sigmaFloor >= 0.0)) die("-sf takes a stdev that is not negative");
    if (nPerms < 0 || nPerms == 1 || nPerms > 1000000) die("-np takes 2 to 1000000 permutations (the first is the design itself)");
    if (permOption && nPerms == 0) die("-ps, -pc, -pf and -two need -np");
    if ((clusterTest || connectivityGiven) && nPerms == 0) die("-ct and -cc need -np");
    if (tfceTest != 0 && tfceTest != 1) die("-tf takes 1 (or 0)");
    if ((tfceTest || tfceOption) && nPerms == 0) die("-tf, -tfd, -tfe and -tfh need -np");
    if (tfceOption && !tfceTest) die("-tfd, -tfe and -tfh need -tf 1");
    if (connectivityGiven && !clusterTest && !tfceTest) die("-cc needs -ct or -tf 1");
    if (tfceTest && (!((float)tfceStep > 0.0f) || !std::isfinite((float)tfceStep))) die("-tfd takes a step that is finite and above 0");
    if (tfceTest && tfceE != 0.5 && tfceE != 1.0) die("-tfe takes 0.5 or 1");
    if (tfceTest && tfceH != 1.0 && tfceH != 2.0) die("-tfh takes 1 or 2");
    if (clusterTest && (!(clusterThreshold >= 0.0) || !std::isfinite((float)clusterThreshold))) die("-ct takes a threshold that is finite and not negative");
    if (connectivity != 6 && connectivity != 18 && connectivity != 26) die("-cc takes 6, 18 or 26");
    if (planesGiven && planesOption < 1) die("-rp takes a number of planes, at least 1");
    {
        char *end = nullptr;
        fwhm = std::strtod(fwhmText.c_str(), &end);
        if (fwhmText.empty() || *end || !(fwhm >= 0.0) || !std::isfinite(fwhm)) die("-s takes a FWHM in mm that is finite and not negative, not '" + fwhmText + "'");
    }
    const double smoothSigma = fwhm / FROG_SMOOTH_FWHM;
    const auto design = read_table(positional[2], "the design");
    const size_t n = design.size(), p = design[0].size();
    if (n > FROG_GLM_MAX_IMAGES) die("at most " + std::to_string(FROG_GLM_MAX_IMAGES) + " images");
    if (p > FROG_GLM_MAX_COLUMNS) die("at most " + std::to_string(FROG_GLM_MAX_COLUMNS) + " design columns");
    if (n <= p) die("the design needs more rows than columns");
    std::vector<double> X(n * p);
    for (size_t i = 0; i < n; i++) std::copy(design[i].begin(), design[i].end(), X.begin() + i * p);
    std::vector<double> contrasts;
    if (!contrastsPath.empty()) {
        const auto rows = read_table(contrastsPath, "the contrasts");
        if (rows[0].size() != p) die(contrastsPath + " has " + std::to_string(rows[0].size()) + " columns for a design of " + std::to_string(p));
        for (const auto &r : rows) contrasts.insert(contrasts.end(), r.begin(), r.end());
    } else {
        for (size_t j = 0; j < p; j++) {
            bool constant = true;
            for (size_t i = 1; i < n; i++) constant = constant && X[i * p + j] == X[j];
            if (constant) continue;
            contrasts.resize(contrasts.size() + p, 0.0);
            contrasts[contrasts.size() - p + j] = 1.0;
        }
        if (contrasts.empty()) die("every design column is constant: give the contrasts with -c");
    }
    const size_t n_c = contrasts.size() / p;
    if (n_c > FROG_GLM_MAX_CONTRASTS) die("at most " + std::to_string(FROG_GLM_MAX_CONTRASTS) + " contrasts");
    uint32_t columns = 0;
    if (!columnList.empty()) {
        for (size_t at = 0; at <= columnList.size();) {
            const size_t comma = std::min(columnList.find(',', at), columnList.size());
            const std::string text = columnList.substr(at, comma - at);
            char *end = nullptr;
            const long j = std::strtol(text.c_str(), &end, 10);
            if (text.empty() || *end || j < 0 || j >= (long)p) die("-pc takes comma-separated column indices below " + std::to_string(p) + ", not '" + text + "'");
            columns |= 1u << j;
            at = comma + 1;
        }
    } else {
        for (size_t c = 0; c < n_c; c++)
            for (size_t j = 0; j < p; j++) if (contrasts[c * p + j] != 0.0) columns |= 1u << j;
    }
    if (nPerms && !columns) die("no column to permute: every contrast is zero");
    std::vector<std::string> volumes, masks;
    if (!volumeList.empty()) {
        if (!read_list(volumeList, volumes)) die("cannot read the volume list " + volumeList);
        if (volumes.size() != n) die(volumeList + " holds " + std::to_string(volumes.size()) + " volumes for " + std::to_string(n) + " design rows");
    }
    if (!maskList.empty()) {
        if (!read_list(maskList, masks)) die("cannot read the mask list " + maskList);
        if (masks.size() != n) die(maskList + " holds " + std::to_string(masks.size()) + " masks for " + std::to_string(n) + " design rows");
    }
    frog_volume grid;
    if (frog_bbox_grid(positional[0].c_str(), atof(positional[1].c_str()), &grid))
        die("cannot read a bounding box from " + positional[0] + " (or spacing " + positional[1] + " is not positive)");
    uint32_t radius[3] = { 0, 0, 0 };
    for (int k = 0; k < 3 && smoothSigma > 0.0; k++)
        if (frog_smooth_taps(smoothSigma, grid.spacing[k], &radius[k], nullptr)) die("-s " + fwhmText + ": " + frog_last_error());
    ChainArguments transforms;
    const auto inverse = inverse_transforms(transforms, transformsDir, n);
    std::vector<frog_volume> supports(volumes.size());
    for (size_t i = 0; i < volumes.size(); i++) {
        if (!peek_header(volumes[i]).ok) die("cannot read volume " + volumes[i]);
        supports[i] = frog_volume{};
        if (!images && frog_volume_geometry(volumes[i].c_str(), supports[i].dims, supports[i].spacing, supports[i].origin))
            die("cannot read the geometry of " + volumes[i]);
    }
    for (const auto &m : masks) {
        const VolumeHeader h = peek_header(m);
        if (!h.ok) die("cannot read mask " + m);
        if (h.is_float) die(m + " is a float volume: masks have an integer type");
    }
    const size_t plane = (size_t)grid.dims[0] * grid.dims[1], total = plane * grid.dims[2];
    std::vector<uint8_t> region;
    if (!regionPath.empty()) {
        int status = 0;
        frog_volume_file *f = frog_volume_read(regionPath.c_str(), &status);
        if (!f) die("cannot read the region mask " + regionPath);
        frog_volume v;
        frog_volume_view(f, &v);
        if (v.dims[0] != grid.dims[0] || v.dims[1] != grid.dims[1] || v.dims[2] != grid.dims[2]) die(regionPath + " is not on the grid");
        if (v.dtype == FROG_V_F32 || v.dtype == FROG_V_F64) die(regionPath + " is a float volume: masks have an integer type");
        region.resize(total);
        const size_t bytes = frog_volume_voxel_bytes(v.dtype);
        const unsigned char *data = (const unsigned char *)v.data;
        for (size_t i = 0; i < total; i++) {
            bool on = false;
            for (size_t b = 0; b < bytes; b++) on = on || data[i * bytes + b] != 0;
            region[i] = on;
        }
        frog_volume_free(f);
    }
    frog_clusters *sink = nullptr;
    if (clusterTest && frog_clusters_create(&grid, (uint32_t)nPerms, (uint32_t)n_c, twoSided == 1, (float)clusterThreshold, connectivity, device, &sink))
        die(frog_last_error());
    frog_tfce *enhance = nullptr;
    if (tfceTest && frog_tfce_create(&grid, (uint32_t)nPerms, (uint32_t)n_c, twoSided == 1, (float)tfceStep, tfceE, tfceH, connectivity, device, &enhance))
        die(frog_last_error());
    begin_output(outDir, n, "images", grid);

    auto t0 = clk::now();
    std::vector<frog_chain *> chains = create_chains(inverse, device);
    uint32_t planes = 0;
    if (smoothSigma > 0.0 ? frog_glm_smooth_planes(&grid, (uint32_t)n, smoothSigma, device, &planes) : frog_glm_planes(&grid, (uint32_t)n, device, &planes))
        die(frog_last_error());
    if (planesGiven && (uint64_t)planesOption < planes) planes = (uint32_t)planesOption;
    const uint32_t depth = grid.dims[2], slabs = (depth + planes - 1) / planes;
    std::cout << "stats : " << slabs << (slabs == 1 ? " slab of " : " slabs of ") << planes << " planes, " << p << " columns, " << n_c << " contrasts, "
              << nPerms << " permutations";
    if (smoothSigma > 0.0)
        std::cout << ", smoothed: FWHM " << fwhm << " mm, sigma " << smoothSigma << " mm, radii " << radius[0] << " " << radius[1] << " " << radius[2] << " voxels";
    std::cout << std::endl;
    std::vector<uint32_t> perm;
    std::vector<int8_t> sign;
    if (nPerms) {
        perm.resize((size_t)nPerms * n);
        sign.resize((size_t)nPerms * n);
        if (frog_glm_draw((uint32_t)n, (uint32_t)nPerms, seed, 1, flips == 1, perm.data(), sign.data())) die(frog_last_error());
    }
    times.setup_s = seconds(t0);

    int threads = 1;
    size_t window = 1;
    frog::volume_stream_shape(n, &threads, &window);
    if (!masks.empty()) threads = std::max(1, threads / 2);
    std::vector<float> beta(p * total), sigma(total), marker(total), t(n_c * total), slabBeta, slabT;
    std::vector<uint16_t> count(total);
    std::vector<float> maxT((size_t)nPerms * n_c, -INFINITY), minT((size_t)nPerms * n_c, INFINITY), slabMax(maxT.size()), slabMin(minT.size());
    double read_s = 0;
    for (uint32_t first = 0; first < depth; first += planes) {
        const uint32_t count_planes = std::min(planes, depth - first);
        const size_t slabVoxels = plane * count_planes, at = plane * first;
        frog_glm *glm = nullptr;
        t0 = clk::now();
        if (frog_glm_create(&grid, first, count_planes, (uint32_t)n, (uint32_t)p, X.data(), device, &glm)) die(frog_last_error());
        if (smoothSigma > 0.0 && frog_glm_smooth(glm, smoothSigma)) die(frog_last_error());
        times.device_s += seconds(t0);
        std::unique_ptr<frog::VolumeStream> stream(images ? new frog::VolumeStream(volumes, threads, window) : nullptr);
        std::unique_ptr<frog::VolumeStream> maskStream(masks.empty() ? nullptr : new frog::VolumeStream(masks, threads, window));
        for (size_t i = 0; i < n; i++) {
            double waited = 0;
            const frog_volume *mask = nullptr;
            if (maskStream) {
                frog::VolumeStream::Item &m = maskStream->get(i, &waited);
                times.waited_s += waited;
                if (!m.file) die("cannot read mask " + masks[i]);
                mask = &m.view;
            }
            if (images) {
                frog::VolumeStream::Item &it = stream->get(i, &waited);
                times.waited_s += waited;
                if (!it.file) die("cannot read volume " + volumes[i]);
                t0 = clk::now();
                if (frog_glm_add(glm, chains[i], &it.view, mask, 1, 0.0)) die(volumes[i] + ": " + frog_last_error());
                times.device_s += seconds(t0);
                stream->release(i);
            } else {
                t0 = clk::now();
                if (frog_glm_add_jacobian(glm, chains[i], supports.empty() ? nullptr : &supports[i], mask, logMode))
                    die("transform " + std::to_string(i) + ": " + frog_last_error());
                times.device_s += seconds(t0);
            }
            if (maskStream) maskStream->release(i);
        }
        if (stream) read_s += stream->read_seconds();
        if (maskStream) read_s += maskStream->read_seconds();
        t0 = clk::now();
        const uint8_t *slabRegion = region.empty() ? nullptr : region.data() + at;
        slabBeta.resize(p * slabVoxels);
        slabT.resize(n_c * slabVoxels);
        if (frog_glm_finish(glm, (uint32_t)n_c, contrasts.data(), (uint32_t)minCount, sigmaFloor, slabRegion, fill, slabBeta.data(), sigma.data() + at,
                            slabT.data(), count.data() + at)) die(frog_last_error());
        // a residual stdev is never -1: the voxels that were not fit
        if (frog_glm_finish(glm, 0, nullptr, (uint32_t)minCount, sigmaFloor, slabRegion, -1.0f, nullptr, marker.data() + at, nullptr, nullptr)) die(frog_last_error());
        for (size_t j = 0; j < p; j++) std::memcpy(beta.data() + j * total + at, slabBeta.data() + j * slabVoxels, slabVoxels * sizeof(float));
        for (size_t c = 0; c < n_c; c++) std::memcpy(t.data() + c * total + at, slabT.data() + c * slabVoxels, slabVoxels * sizeof(float));
        if (nPerms) {
            const int8_t *signs = flips == 1 ? sign.data() : nullptr;
            if (sink ? frog_glm_permute_clusters(glm, (uint32_t)n_c, contrasts.data(), (uint32_t)minCount, sigmaFloor, slabRegion, columns, (uint32_t)nPerms,
                                                 perm.data(), signs, 0, sink, slabMax.data(), slabMin.data())
                     : frog_glm_permute(glm, (uint32_t)n_c, contrasts.data(), (uint32_t)minCount, sigmaFloor, slabRegion, columns, (uint32_t)nPerms, perm.data(),
                                        signs, slabMax.data(), slabMin.data())) die(frog_last_error());
            // the same adds fill the second sink; the extrema are the same bits and are taken once
            if (enhance && frog_glm_permute_tfce(glm, (uint32_t)n_c, contrasts.data(), (uint32_t)minCount, sigmaFloor, slabRegion, columns, (uint32_t)nPerms,
                                                 perm.data(), signs, 0, enhance, nullptr, nullptr)) die(frog_last_error());
            for (size_t e = 0; e < maxT.size(); e++) {
                if (float_key(slabMax[e]) > float_key(maxT[e])) maxT[e] = slabMax[e];
                if (float_key(slabMin[e]) < float_key(minT[e])) minT[e] = slabMin[e];
            }
        }
        times.device_s += seconds(t0);
        frog_glm_destroy(glm);
    }
    for (frog_chain *c : chains) frog_chain_destroy(c);
    // the cluster-extent test: every slot's largest extent, and the observed map's labels, the negative side's after the positive's
    const uint32_t sides = twoSided == 1 ? 2 : 1;
    std::vector<uint32_t> slotExtent, clusterLabels, sideLabels;
    std::vector<std::vector<int>> clusterSign(n_c);
    if (sink) {
        t0 = clk::now();
        slotExtent.resize((size_t)nPerms * n_c * sides);
        if (frog_clusters_finish(sink, slotExtent.data())) die(frog_last_error());
        clusterLabels.assign(n_c * total, 0);
        sideLabels.resize(total);
        for (size_t c = 0; c < n_c; c++)
            for (uint32_t side = 0; side < sides; side++) {
                uint32_t found = 0;
                if (frog_clusters_labels(sink, 0, (uint32_t)c, (int)side, sideLabels.data(), &found)) die(frog_last_error());
                const uint32_t before = (uint32_t)clusterSign[c].size();
                for (size_t v = 0; v < total; v++) if (sideLabels[v]) clusterLabels[c * total + v] = sideLabels[v] + before;
                clusterSign[c].resize(before + found, side ? -1 : 1);
            }
        times.device_s += seconds(t0);
        frog_clusters_destroy(sink);
    }
    // threshold-free cluster enhancement: every slot's largest value, and the observed maps, the negative side's negated
    std::vector<float> slotTfce, tfceMap, sideMap;
    if (enhance) {
        t0 = clk::now();
        slotTfce.resize((size_t)nPerms * n_c * sides);
        if (frog_tfce_finish(enhance, slotTfce.data())) die(frog_last_error());
        tfceMap.resize(n_c * total);
        sideMap.resize(total);
        for (size_t c = 0; c < n_c; c++) {
            if (frog_tfce_map(enhance, 0, (uint32_t)c, 0, tfceMap.data() + c * total)) die(frog_last_error());
            if (sides == 2) {
                if (frog_tfce_map(enhance, 0, (uint32_t)c, 1, sideMap.data())) die(frog_last_error());
                for (size_t v = 0; v < total; v++) tfceMap[c * total + v] -= sideMap[v];       // a voxel has at most one side
            }
        }
        times.device_s += seconds(t0);
        frog_tfce_destroy(enhance);
    }

    // ---- the files
    t0 = clk::now();
    auto write = [&](const std::string &name, int dtype, void *data) {
        grid.dtype = dtype;
        grid.data = data;
        const std::string path = outDir + "/" + name;
        if (frog_volume_write(path.c_str(), &grid)) die("cannot write " + path);
    };
    for (size_t j = 0; j < p; j++) write("beta_" + std::to_string(j) + ".nii.gz", FROG_V_F32, beta.data() + j * total);
    write("sigma.nii.gz", FROG_V_F32, sigma.data());
    write("count.nii.gz", FROG_V_U16, count.data());
    for (size_t c = 0; c < n_c; c++) write("t_" + std::to_string(c) + ".nii.gz", FROG_V_F32, t.data() + c * total);
    std::vector<double> threshold(n_c, NAN);
    std::vector<uint64_t> beyond(n_c, 0);
    if (nPerms) {
        std::ofstream csv(outDir + "/maxt.csv");
        csv << "permutation,contrast,max,min\n";
        for (long k = 0; k < nPerms; k++)
            for (size_t c = 0; c < n_c; c++) csv << k << "," << c << "," << csv_float(maxT[k * n_c + c]) << "," << csv_float(minT[k * n_c + c]) << "\n";
        csv.close();
        if (!csv) die("cannot write " + outDir + "/maxt.csv");
        std::vector<float> pmap(total), null((size_t)nPerms - 1);
        for (size_t c = 0; c < n_c; c++) {
            for (long k = 1; k < nPerms; k++) {
                const float hi = maxT[k * n_c + c], lo = -minT[k * n_c + c];
                null[k - 1] = twoSided == 1 && lo > hi ? lo : hi;
            }
            std::sort(null.begin(), null.end());
            // p < 0.05 iff 20 (1 + exceedances) < nPerms: the largest such count, and the null maximum a t must exceed for it
            const long allowed = (nPerms - 1) / 20 - 1;         // exceedances allowed; < 0: none gives p < 0.05
            threshold[c] = allowed < 0 ? INFINITY : (allowed >= (long)null.size() ? -INFINITY : (double)null[null.size() - 1 - allowed]);
            for (size_t v = 0; v < total; v++) {
                float value = t[c * total + v];
                if (twoSided == 1) value = std::fabs(value);
                float pv = 1.0f;
                if (marker[v] != -1.0f && !std::isnan(value)) {
                    const size_t exceed = null.end() - std::lower_bound(null.begin(), null.end(), value);
                    pv = (float)((double)(1 + exceed) / (double)nPerms);
                    if (20 * (1 + (long)exceed) < nPerms) beyond[c]++;
                }
                pmap[v] = pv;
            }
            write("fwe_p_" + std::to_string(c) + ".nii.gz", FROG_V_F32, pmap.data());
        }
    }
    if (clusterTest) {
        std::ofstream csv(outDir + "/maxextent.csv"), table(outDir + "/clusters.csv");
        csv << "permutation,contrast,extent\n";
        table << "contrast,cluster,sign,voxels,peak_t,peak_x,peak_y,peak_z,p_fwe\n";
        auto nullExtent = [&](long k, size_t c) {
            const uint32_t *e = slotExtent.data() + ((size_t)k * n_c + c) * sides;
            return sides == 2 ? std::max(e[0], e[1]) : e[0];
        };
        for (long k = 0; k < nPerms; k++)
            for (size_t c = 0; c < n_c; c++) csv << k << "," << c << "," << nullExtent(k, c) << "\n";
        csv.close();
        if (!csv) die("cannot write " + outDir + "/maxextent.csv");
        std::vector<float> pmap(total);
        std::vector<uint32_t> null((size_t)nPerms - 1);
        for (size_t c = 0; c < n_c; c++) {
            const size_t found = clusterSign[c].size();
            const uint32_t *labels = clusterLabels.data() + c * total;
            std::vector<uint64_t> voxels(found + 1, 0);
            std::vector<size_t> peak(found + 1, total);
            for (size_t v = 0; v < total; v++) {
                const uint32_t l = labels[v];
                if (!l) continue;
                voxels[l]++;
                if (peak[l] == total || std::fabs(t[c * total + v]) > std::fabs(t[c * total + peak[l]])) peak[l] = v;
            }
            for (long k = 1; k < nPerms; k++) null[k - 1] = nullExtent(k, c);
            std::sort(null.begin(), null.end());
            std::vector<float> pOf(found + 1, 1.0f);
            for (size_t l = 1; l <= found; l++) {
                const size_t reach = null.end() - std::lower_bound(null.begin(), null.end(), (uint32_t)voxels[l]);
                pOf[l] = (float)((double)(1 + reach) / (double)nPerms);
                table << c << "," << l << "," << clusterSign[c][l - 1] << "," << voxels[l] << "," << csv_float(t[c * total + peak[l]]) << "," << peak[l] % grid.dims[0]
                      << "," << (peak[l] / grid.dims[0]) % grid.dims[1] << "," << peak[l] / plane << "," << csv_float(pOf[l]) << "\n";
            }
            for (size_t v = 0; v < total; v++) pmap[v] = pOf[labels[v]];
            write("clusters_" + std::to_string(c) + ".nii.gz", FROG_V_I32, clusterLabels.data() + c * total);
            write("cluster_p_" + std::to_string(c) + ".nii.gz", FROG_V_F32, pmap.data());
        }
        table.close();
        if (!table) die("cannot write " + outDir + "/clusters.csv");
    }
    if (tfceTest) {
        std::ofstream csv(outDir + "/maxtfce.csv"), table(outDir + "/tfce.csv");
        csv << "permutation,contrast,max_tfce\n";
        table << "contrast,peak_tfce,peak_x,peak_y,peak_z,threshold_p05,voxels_p05\n";
        auto nullTfce = [&](long k, size_t c) {
            const float *e = slotTfce.data() + ((size_t)k * n_c + c) * sides;
            return sides == 2 ? std::max(e[0], e[1]) : e[0];
        };
        for (long k = 0; k < nPerms; k++)
            for (size_t c = 0; c < n_c; c++) csv << k << "," << c << "," << csv_float(nullTfce(k, c)) << "\n";
        csv.close();
        if (!csv) die("cannot write " + outDir + "/maxtfce.csv");
        std::vector<float> pmap(total), null((size_t)nPerms - 1);
        for (size_t c = 0; c < n_c; c++) {
            for (long k = 1; k < nPerms; k++) null[k - 1] = nullTfce(k, c);
            std::sort(null.begin(), null.end());
            // maxt.csv's rule: the largest null maximum a value must exceed for p < 0.05
            const long allowed = (nPerms - 1) / 20 - 1;
            const double limit = allowed < 0 ? INFINITY : (allowed >= (long)null.size() ? -INFINITY : (double)null[null.size() - 1 - allowed]);
            const float *map = tfceMap.data() + c * total;
            uint64_t past = 0;
            size_t peak = total;
            for (size_t v = 0; v < total; v++) {
                const float value = std::fabs(map[v]);
                float pv = 1.0f;
                if (value != 0.0f) {
                    const size_t exceed = null.end() - std::lower_bound(null.begin(), null.end(), value);
                    pv = (float)((double)(1 + exceed) / (double)nPerms);
                    if (20 * (1 + (long)exceed) < nPerms) past++;
                    if (peak == total || value > std::fabs(map[peak])) peak = v;
                }
                pmap[v] = pv;
            }
            table << c << ",";
            if (peak < total) table << csv_float(map[peak]) << "," << peak % grid.dims[0] << "," << (peak / grid.dims[0]) % grid.dims[1] << "," << peak / plane;
            else table << "nan,,,";
            table << "," << csv_float((float)limit) << "," << past << "\n";
            write("tfce_" + std::to_string(c) + ".nii.gz", FROG_V_F32, tfceMap.data() + c * total);
            write("tfce_p_" + std::to_string(c) + ".nii.gz", FROG_V_F32, pmap.data());
        }
        table.close();
        if (!table) die("cannot write " + outDir + "/tfce.csv");
    }
    {
        std::ofstream csv(outDir + "/glm.csv");
        csv << "contrast,fit_voxels,peak_t,peak_x,peak_y,peak_z,threshold_p05,voxels_p05\n";
        for (size_t c = 0; c < n_c; c++) {
            uint64_t fit = 0;
            size_t peak = total;
            for (size_t v = 0; v < total; v++) {
                const float value = t[c * total + v];
                if (marker[v] == -1.0f || std::isnan(value)) continue;
                fit++;
                const float best = peak < total ? t[c * total + peak] : 0.0f;
                if (peak == total || (twoSided == 1 ? std::fabs(value) > std::fabs(best) : value > best)) peak = v;
            }
            csv << c << "," << fit << ",";
            if (peak < total) csv << csv_float(t[c * total + peak]) << "," << peak % grid.dims[0] << "," << (peak / grid.dims[0]) % grid.dims[1] << "," << peak / plane;
            else csv << "nan,,,";
            csv << "," << (std::isnan(threshold[c]) ? std::string("nan") : csv_float((float)threshold[c])) << "," << beyond[c] << "\n";
        }
        csv.close();
        if (!csv) die("cannot write " + outDir + "/glm.csv");
    }
    times.write_s += seconds(t0);
    times.print(read_s, images || !masks.empty() ? threads : 0);
    return 0;
}
