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
#include "inference.h"
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

using frog::csv_float;

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

// ---- the options -----------------------------------------------------------------------------------------------------------------

// the command line as it was given, before any check
struct Options {
    std::vector<std::string> positional;
    std::string transformsDir = "transforms", outDir = ".", contrastsPath, valueName = "logjacobian", volumeList, maskList, regionPath, columnList;
    std::string fwhmText = "0";
    int device = 0, flips = 0, twoSided = 0, connectivity = 26, tfceTest = 0;
    long minCount = 1, nPerms = 0, planesOption = 0;
    unsigned long long seed = 0;
    double sigmaFloor = 0, clusterThreshold = 0, tfceStep = 0.1, tfceE = 0.5, tfceH = 2;
    float fill = 0;
    bool planesGiven = false, permOption = false, clusterTest = false, connectivityGiven = false, tfceOption = false;

    uint32_t sides() const { return twoSided == 1 ? 2 : 1; }
};

Options parse_options(int argc, char *argv[])
{
    Options o;
    int a = positional_arguments(argc, argv, 1, { "-c", "-td", "-o", "-v", "-vl", "-ml", "-m", "-mc", "-sf", "-f", "-np", "-ps", "-pc", "-pf", "-two", "-ct", "-cc", "-tf", "-tfd", "-tfe", "-tfh", "-s", "-rp", "-dev" },
                                 o.positional);
    for (; a < argc; a += 2) {
        const char *key = argv[a], *value = a + 1 < argc ? argv[a + 1] : "";
        if (std::strcmp(key, "-c") == 0) o.contrastsPath = value;
        else if (std::strcmp(key, "-td") == 0) o.transformsDir = value;
        else if (std::strcmp(key, "-o") == 0) o.outDir = value;
        else if (std::strcmp(key, "-v") == 0) o.valueName = value;
        else if (std::strcmp(key, "-vl") == 0) o.volumeList = value;
        else if (std::strcmp(key, "-ml") == 0) o.maskList = value;
        else if (std::strcmp(key, "-m") == 0) o.regionPath = value;
        else if (std::strcmp(key, "-mc") == 0) o.minCount = atol(value);
        else if (std::strcmp(key, "-sf") == 0) o.sigmaFloor = atof(value);
        else if (std::strcmp(key, "-f") == 0) o.fill = (float)atof(value);
        else if (std::strcmp(key, "-np") == 0) o.nPerms = atol(value);
        else if (std::strcmp(key, "-ps") == 0) { o.seed = std::strtoull(value, nullptr, 10); o.permOption = true; }
        else if (std::strcmp(key, "-pc") == 0) { o.columnList = value; o.permOption = true; }
        else if (std::strcmp(key, "-pf") == 0) { o.flips = atoi(value); o.permOption = true; }
        else if (std::strcmp(key, "-two") == 0) { o.twoSided = atoi(value); o.permOption = true; }
        else if (std::strcmp(key, "-ct") == 0) { o.clusterThreshold = atof(value); o.clusterTest = true; }
        else if (std::strcmp(key, "-cc") == 0) { o.connectivity = atoi(value); o.connectivityGiven = true; }
        else if (std::strcmp(key, "-tf") == 0) o.tfceTest = atoi(value);
        else if (std::strcmp(key, "-tfd") == 0) { o.tfceStep = atof(value); o.tfceOption = true; }
        else if (std::strcmp(key, "-tfe") == 0) { o.tfceE = atof(value); o.tfceOption = true; }
        else if (std::strcmp(key, "-tfh") == 0) { o.tfceH = atof(value); o.tfceOption = true; }
        else if (std::strcmp(key, "-s") == 0) o.fwhmText = value;
        else if (std::strcmp(key, "-rp") == 0) { o.planesOption = atol(value); o.planesGiven = true; }
        else if (std::strcmp(key, "-dev") == 0) o.device = atoi(value);
        else die(std::string("unknown option ") + key);
    }
    return o;
}

// ---- the checks: everything is checked before the first output ---------------------------------------------------------------------

// what the checks load and work out: the model, the grid, and what each image is read from
struct Inputs {
    bool images = false, logMode = false;
    double fwhm = 0, smoothSigma = 0;
    size_t n = 0, p = 0, n_c = 0;                   // images, design columns, contrasts
    std::vector<double> X, contrasts;
    uint32_t columns = 0;                           // the columns the permutations move, as bits
    std::vector<std::string> volumes, masks;
    frog_volume grid;
    size_t plane = 0, total = 0;
    uint32_t radius[3] = { 0, 0, 0 };
    ChainArguments transforms;
    std::vector<std::vector<frog_chain_link>> inverse;
    std::vector<frog_volume> supports;
    std::vector<uint8_t> region;
};

// the options by themselves
void check_options(const Options &o, Inputs &in)
{
    in.images = o.valueName == "images";
    in.logMode = o.valueName == "logjacobian";
    if (!in.images && !in.logMode && o.valueName != "jacobian") die("-v takes jacobian, logjacobian or images, not '" + o.valueName + "'");
    if (in.images && o.volumeList.empty()) die("-v images needs the volumes: -vl volumes.txt");
    if (o.minCount < 1 || o.minCount > 65535) die("-mc takes a count from 1 to 65535");
    if (!(o.sigmaFloor >= 0.0)) die("-sf takes a stdev that is not negative");
    if (o.nPerms < 0 || o.nPerms == 1 || o.nPerms > 1000000) die("-np takes 2 to 1000000 permutations (the first is the design itself)");
    if (o.permOption && o.nPerms == 0) die("-ps, -pc, -pf and -two need -np");
    if ((o.clusterTest || o.connectivityGiven) && o.nPerms == 0) die("-ct and -cc need -np");
    if (o.tfceTest != 0 && o.tfceTest != 1) die("-tf takes 1 (or 0)");
    if ((o.tfceTest || o.tfceOption) && o.nPerms == 0) die("-tf, -tfd, -tfe and -tfh need -np");
    if (o.tfceOption && !o.tfceTest) die("-tfd, -tfe and -tfh need -tf 1");
    if (o.connectivityGiven && !o.clusterTest && !o.tfceTest) die("-cc needs -ct or -tf 1");
    if (o.tfceTest && (!((float)o.tfceStep > 0.0f) || !std::isfinite((float)o.tfceStep))) die("-tfd takes a step that is finite and above 0");
    if (o.tfceTest && o.tfceE != 0.5 && o.tfceE != 1.0) die("-tfe takes 0.5 or 1");
    if (o.tfceTest && o.tfceH != 1.0 && o.tfceH != 2.0) die("-tfh takes 1 or 2");
    if (o.clusterTest && (!(o.clusterThreshold >= 0.0) || !std::isfinite((float)o.clusterThreshold))) die("-ct takes a threshold that is finite and not negative");
    if (o.connectivity != 6 && o.connectivity != 18 && o.connectivity != 26) die("-cc takes 6, 18 or 26");
    if (o.planesGiven && o.planesOption < 1) die("-rp takes a number of planes, at least 1");
    char *end = nullptr;
    in.fwhm = std::strtod(o.fwhmText.c_str(), &end);
    if (o.fwhmText.empty() || *end || !(in.fwhm >= 0.0) || !std::isfinite(in.fwhm)) die("-s takes a FWHM in mm that is finite and not negative, not '" + o.fwhmText + "'");
    in.smoothSigma = in.fwhm / FROG_SMOOTH_FWHM;
}

// the design, the contrasts and the columns that move
void load_model(const Options &o, Inputs &in)
{
    const auto design = read_table(o.positional[2], "the design");
    const size_t n = in.n = design.size(), p = in.p = design[0].size();
    if (n > FROG_GLM_MAX_IMAGES) die("at most " + std::to_string(FROG_GLM_MAX_IMAGES) + " images");
    if (p > FROG_GLM_MAX_COLUMNS) die("at most " + std::to_string(FROG_GLM_MAX_COLUMNS) + " design columns");
    if (n <= p) die("the design needs more rows than columns");
    std::vector<double> &X = in.X, &contrasts = in.contrasts;
    X.resize(n * p);
    for (size_t i = 0; i < n; i++) std::copy(design[i].begin(), design[i].end(), X.begin() + i * p);
    if (!o.contrastsPath.empty()) {
        const auto rows = read_table(o.contrastsPath, "the contrasts");
        if (rows[0].size() != p) die(o.contrastsPath + " has " + std::to_string(rows[0].size()) + " columns for a design of " + std::to_string(p));
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
    const size_t n_c = in.n_c = contrasts.size() / p;
    if (n_c > FROG_GLM_MAX_CONTRASTS) die("at most " + std::to_string(FROG_GLM_MAX_CONTRASTS) + " contrasts");
    if (!o.columnList.empty()) {
        for (size_t at = 0; at <= o.columnList.size();) {
            const size_t comma = std::min(o.columnList.find(',', at), o.columnList.size());
            const std::string text = o.columnList.substr(at, comma - at);
            char *end = nullptr;
            const long j = std::strtol(text.c_str(), &end, 10);
            if (text.empty() || *end || j < 0 || j >= (long)p) die("-pc takes comma-separated column indices below " + std::to_string(p) + ", not '" + text + "'");
            in.columns |= 1u << j;
            at = comma + 1;
        }
    } else {
        for (size_t c = 0; c < n_c; c++)
            for (size_t j = 0; j < p; j++) if (contrasts[c * p + j] != 0.0) in.columns |= 1u << j;
    }
    if (o.nPerms && !in.columns) die("no column to permute: every contrast is zero");
}

// the -m volume as one flag per grid voxel
void load_region(const std::string &regionPath, Inputs &in)
{
    int status = 0;
    frog_volume_file *f = frog_volume_read(regionPath.c_str(), &status);
    if (!f) die("cannot read the region mask " + regionPath);
    frog_volume v;
    frog_volume_view(f, &v);
    if (v.dims[0] != in.grid.dims[0] || v.dims[1] != in.grid.dims[1] || v.dims[2] != in.grid.dims[2]) die(regionPath + " is not on the grid");
    if (v.dtype == FROG_V_F32 || v.dtype == FROG_V_F64) die(regionPath + " is a float volume: masks have an integer type");
    in.region.resize(in.total);
    const size_t bytes = frog_volume_voxel_bytes(v.dtype);
    const unsigned char *data = (const unsigned char *)v.data;
    for (size_t i = 0; i < in.total; i++) {
        bool on = false;
        for (size_t b = 0; b < bytes; b++) on = on || data[i * bytes + b] != 0;
        in.region[i] = on;
    }
    frog_volume_free(f);
}

// the lists, the grid, the transforms, and the header of every volume and mask
void load_images(const Options &o, Inputs &in)
{
    const size_t n = in.n;
    if (!o.volumeList.empty()) {
        if (!read_list(o.volumeList, in.volumes)) die("cannot read the volume list " + o.volumeList);
        if (in.volumes.size() != n) die(o.volumeList + " holds " + std::to_string(in.volumes.size()) + " volumes for " + std::to_string(n) + " design rows");
    }
    if (!o.maskList.empty()) {
        if (!read_list(o.maskList, in.masks)) die("cannot read the mask list " + o.maskList);
        if (in.masks.size() != n) die(o.maskList + " holds " + std::to_string(in.masks.size()) + " masks for " + std::to_string(n) + " design rows");
    }
    if (frog_bbox_grid(o.positional[0].c_str(), atof(o.positional[1].c_str()), &in.grid))
        die("cannot read a bounding box from " + o.positional[0] + " (or spacing " + o.positional[1] + " is not positive)");
    for (int k = 0; k < 3 && in.smoothSigma > 0.0; k++)
        if (frog_smooth_taps(in.smoothSigma, in.grid.spacing[k], &in.radius[k], nullptr)) die("-s " + o.fwhmText + ": " + frog_last_error());
    in.inverse = inverse_transforms(in.transforms, o.transformsDir, n);
    in.supports.resize(in.volumes.size());
    for (size_t i = 0; i < in.volumes.size(); i++) {
        if (!peek_header(in.volumes[i]).ok) die("cannot read volume " + in.volumes[i]);
        in.supports[i] = frog_volume{};
        if (!in.images && frog_volume_geometry(in.volumes[i].c_str(), in.supports[i].dims, in.supports[i].spacing, in.supports[i].origin))
            die("cannot read the geometry of " + in.volumes[i]);
    }
    for (const auto &m : in.masks) {
        const VolumeHeader h = peek_header(m);
        if (!h.ok) die("cannot read mask " + m);
        if (h.is_float) die(m + " is a float volume: masks have an integer type");
    }
    in.plane = (size_t)in.grid.dims[0] * in.grid.dims[1];
    in.total = in.plane * in.grid.dims[2];
    if (!o.regionPath.empty()) load_region(o.regionPath, in);
}

// ---- the fit ---------------------------------------------------------------------------------------------------------------------

// what the slabs share: one chain per image, the planes of a slab, and the permutations' rows
struct Plan {
    std::vector<frog_chain *> chains;
    uint32_t planes = 0;
    std::vector<uint32_t> perm;
    std::vector<int8_t> sign;
};

void set_up(const Options &o, const Inputs &in, Plan &plan)
{
    plan.chains = create_chains(in.inverse, o.device);
    uint32_t &planes = plan.planes;
    if (in.smoothSigma > 0.0 ? frog_glm_smooth_planes(&in.grid, (uint32_t)in.n, in.smoothSigma, o.device, &planes) : frog_glm_planes(&in.grid, (uint32_t)in.n, o.device, &planes))
        die(frog_last_error());
    if (o.planesGiven && (uint64_t)o.planesOption < planes) planes = (uint32_t)o.planesOption;
    const uint32_t slabs = (in.grid.dims[2] + planes - 1) / planes;
    std::cout << "stats : " << slabs << (slabs == 1 ? " slab of " : " slabs of ") << planes << " planes, " << in.p << " columns, " << in.n_c << " contrasts, "
              << o.nPerms << " permutations";
    if (in.smoothSigma > 0.0)
        std::cout << ", smoothed: FWHM " << in.fwhm << " mm, sigma " << in.smoothSigma << " mm, radii " << in.radius[0] << " " << in.radius[1] << " " << in.radius[2] << " voxels";
    std::cout << std::endl;
    if (o.nPerms) {
        plan.perm.resize((size_t)o.nPerms * in.n);
        plan.sign.resize((size_t)o.nPerms * in.n);
        if (frog_glm_draw((uint32_t)in.n, (uint32_t)o.nPerms, o.seed, 1, o.flips == 1, plan.perm.data(), plan.sign.data())) die(frog_last_error());
    }
}

// the maps over the whole grid, and the permutations' extrema over it ([permutation * n_c + contrast])
struct Fit {
    std::vector<float> beta, sigma, marker, t, maxT, minT;     // marker: -1 where the voxel was not fit
    std::vector<uint16_t> count;
    double read_s = 0;
    int threads = 1;
    size_t window = 1;
};

// every image's map into one slab's accumulator, in the order of the design's rows
void add_images(const Inputs &in, const Plan &plan, frog_glm *glm, Fit &fit, PhaseTimes &times)
{
    std::unique_ptr<frog::VolumeStream> stream(in.images ? new frog::VolumeStream(in.volumes, fit.threads, fit.window) : nullptr);
    std::unique_ptr<frog::VolumeStream> maskStream(in.masks.empty() ? nullptr : new frog::VolumeStream(in.masks, fit.threads, fit.window));
    for (size_t i = 0; i < in.n; i++) {
        double waited = 0;
        const frog_volume *mask = nullptr;
        if (maskStream) {
            frog::VolumeStream::Item &m = maskStream->get(i, &waited);
            times.waited_s += waited;
            if (!m.file) die("cannot read mask " + in.masks[i]);
            mask = &m.view;
        }
        if (in.images) {
            frog::VolumeStream::Item &it = stream->get(i, &waited);
            times.waited_s += waited;
            if (!it.file) die("cannot read volume " + in.volumes[i]);
            const auto t0 = clk::now();
            if (frog_glm_add(glm, plan.chains[i], &it.view, mask, 1, 0.0)) die(in.volumes[i] + ": " + frog_last_error());
            times.device_s += seconds(t0);
            stream->release(i);
        } else {
            const auto t0 = clk::now();
            if (frog_glm_add_jacobian(glm, plan.chains[i], in.supports.empty() ? nullptr : &in.supports[i], mask, in.logMode))
                die("transform " + std::to_string(i) + ": " + frog_last_error());
            times.device_s += seconds(t0);
        }
        if (maskStream) maskStream->release(i);
    }
    if (stream) fit.read_s += stream->read_seconds();
    if (maskStream) fit.read_s += maskStream->read_seconds();
}

// One slab's permutations: its extrema into the grid's, and its bits and levels into the sinks.  Each sink takes a pass of
// its own; the extrema are the same bits in both and are taken once.
void permute_slab(const Options &o, const Inputs &in, const Plan &plan, frog_glm *glm, const uint8_t *slabRegion, frog_clusters *sink, frog_tfce *enhance,
                  Fit &fit, std::vector<float> &slabMax, std::vector<float> &slabMin)
{
    const uint32_t n_c = (uint32_t)in.n_c, minCount = (uint32_t)o.minCount, nPerms = (uint32_t)o.nPerms;
    const int8_t *signs = o.flips == 1 ? plan.sign.data() : nullptr;
    if (sink ? frog_glm_permute_clusters(glm, n_c, in.contrasts.data(), minCount, o.sigmaFloor, slabRegion, in.columns, nPerms, plan.perm.data(), signs, 0, sink,
                                         slabMax.data(), slabMin.data())
             : frog_glm_permute(glm, n_c, in.contrasts.data(), minCount, o.sigmaFloor, slabRegion, in.columns, nPerms, plan.perm.data(), signs, slabMax.data(),
                                slabMin.data())) die(frog_last_error());
    if (enhance && frog_glm_permute_tfce(glm, n_c, in.contrasts.data(), minCount, o.sigmaFloor, slabRegion, in.columns, nPerms, plan.perm.data(), signs, 0, enhance,
                                         nullptr, nullptr)) die(frog_last_error());
    for (size_t e = 0; e < fit.maxT.size(); e++) {
        if (float_key(slabMax[e]) > float_key(fit.maxT[e])) fit.maxT[e] = slabMax[e];
        if (float_key(slabMin[e]) < float_key(fit.minT[e])) fit.minT[e] = slabMin[e];
    }
}

// the slab loop: per slab an accumulator, every image's map, the fit, and the permutations
void fit_slabs(const Options &o, const Inputs &in, const Plan &plan, frog_clusters *sink, frog_tfce *enhance, Fit &fit, PhaseTimes &times)
{
    const size_t n = in.n, p = in.p, n_c = in.n_c, plane = in.plane, total = in.total;
    frog::volume_stream_shape(n, &fit.threads, &fit.window);
    if (!in.masks.empty()) fit.threads = std::max(1, fit.threads / 2);
    fit.beta.resize(p * total);
    fit.sigma.resize(total);
    fit.marker.resize(total);
    fit.t.resize(n_c * total);
    fit.count.resize(total);
    fit.maxT.assign((size_t)o.nPerms * n_c, -INFINITY);
    fit.minT.assign((size_t)o.nPerms * n_c, INFINITY);
    std::vector<float> slabBeta, slabT, slabMax(fit.maxT.size()), slabMin(fit.minT.size());
    const uint32_t depth = in.grid.dims[2], minCount = (uint32_t)o.minCount;
    for (uint32_t first = 0; first < depth; first += plan.planes) {
        const uint32_t count_planes = std::min(plan.planes, depth - first);
        const size_t slabVoxels = plane * count_planes, at = plane * first;
        frog_glm *glm = nullptr;
        auto t0 = clk::now();
        if (frog_glm_create(&in.grid, first, count_planes, (uint32_t)n, (uint32_t)p, in.X.data(), o.device, &glm)) die(frog_last_error());
        if (in.smoothSigma > 0.0 && frog_glm_smooth(glm, in.smoothSigma)) die(frog_last_error());
        times.device_s += seconds(t0);
        add_images(in, plan, glm, fit, times);
        t0 = clk::now();
        const uint8_t *slabRegion = in.region.empty() ? nullptr : in.region.data() + at;
        slabBeta.resize(p * slabVoxels);
        slabT.resize(n_c * slabVoxels);
        if (frog_glm_finish(glm, (uint32_t)n_c, in.contrasts.data(), minCount, o.sigmaFloor, slabRegion, o.fill, slabBeta.data(), fit.sigma.data() + at, slabT.data(),
                            fit.count.data() + at)) die(frog_last_error());
        // a residual stdev is never -1: the voxels that were not fit
        if (frog_glm_finish(glm, 0, nullptr, minCount, o.sigmaFloor, slabRegion, -1.0f, nullptr, fit.marker.data() + at, nullptr, nullptr)) die(frog_last_error());
        for (size_t j = 0; j < p; j++) std::memcpy(fit.beta.data() + j * total + at, slabBeta.data() + j * slabVoxels, slabVoxels * sizeof(float));
        for (size_t c = 0; c < n_c; c++) std::memcpy(fit.t.data() + c * total + at, slabT.data() + c * slabVoxels, slabVoxels * sizeof(float));
        if (o.nPerms) permute_slab(o, in, plan, glm, slabRegion, sink, enhance, fit, slabMax, slabMin);
        times.device_s += seconds(t0);
        frog_glm_destroy(glm);
    }
    for (frog_chain *c : plan.chains) frog_chain_destroy(c);
}

// ---- the sinks' read-outs ----------------------------------------------------------------------------------------------------------

// the cluster-extent test: every slot's largest extent, and the observed map's labels, the negative side's after the positive's
struct Clusters {
    std::vector<uint32_t> extent, labels;           // [(permutation * n_c + contrast) * sides + side], [contrast * total + voxel]
    std::vector<std::vector<int>> sign;             // per contrast: +1 or -1 of cluster l at [l - 1]
};

void read_clusters(frog_clusters *sink, const Options &o, const Inputs &in, Clusters &got, PhaseTimes &times)
{
    const auto t0 = clk::now();
    const uint32_t sides = o.sides();
    got.extent.resize((size_t)o.nPerms * in.n_c * sides);
    if (frog_clusters_finish(sink, got.extent.data())) die(frog_last_error());
    got.labels.assign(in.n_c * in.total, 0);
    got.sign.resize(in.n_c);
    std::vector<uint32_t> sideLabels(in.total);
    for (size_t c = 0; c < in.n_c; c++)
        for (uint32_t side = 0; side < sides; side++) {
            uint32_t found = 0;
            if (frog_clusters_labels(sink, 0, (uint32_t)c, (int)side, sideLabels.data(), &found)) die(frog_last_error());
            const uint32_t before = (uint32_t)got.sign[c].size();
            for (size_t v = 0; v < in.total; v++) if (sideLabels[v]) got.labels[c * in.total + v] = sideLabels[v] + before;
            got.sign[c].resize(before + found, side ? -1 : 1);
        }
    times.device_s += seconds(t0);
    frog_clusters_destroy(sink);
}

// threshold-free cluster enhancement: every slot's largest value, and the observed maps, the negative side's negated
struct Enhanced {
    std::vector<float> max, map;                    // [(permutation * n_c + contrast) * sides + side], [contrast * total + voxel]
};

void read_tfce(frog_tfce *enhance, const Options &o, const Inputs &in, Enhanced &got, PhaseTimes &times)
{
    const auto t0 = clk::now();
    const uint32_t sides = o.sides();
    got.max.resize((size_t)o.nPerms * in.n_c * sides);
    if (frog_tfce_finish(enhance, got.max.data())) die(frog_last_error());
    got.map.resize(in.n_c * in.total);
    std::vector<float> sideMap(in.total);
    for (size_t c = 0; c < in.n_c; c++) {
        if (frog_tfce_map(enhance, 0, (uint32_t)c, 0, got.map.data() + c * in.total)) die(frog_last_error());
        if (sides == 2) {
            if (frog_tfce_map(enhance, 0, (uint32_t)c, 1, sideMap.data())) die(frog_last_error());
            for (size_t v = 0; v < in.total; v++) got.map[c * in.total + v] -= sideMap[v];     // a voxel has at most one side
        }
    }
    times.device_s += seconds(t0);
    frog_tfce_destroy(enhance);
}

// ---- the files -------------------------------------------------------------------------------------------------------------------

struct Output {
    std::string dir;
    frog_volume grid;

    std::string path(const std::string &name) const { return dir + "/" + name; }
    void volume(const std::string &name, int dtype, void *data)
    {
        grid.dtype = dtype;
        grid.data = data;
        if (frog_volume_write(path(name).c_str(), &grid)) die("cannot write " + path(name));
    }
    void close(std::ofstream &csv, const std::string &name) const
    {
        if (!frog::csv_close(csv)) die("cannot write " + path(name));
    }
};

// the null distribution of contrast c: of(k) under the permutations k = 1..nPerms-1
template <class T, class Of>
frog::NullDistribution<T> null_of(long nPerms, Of of)
{
    std::vector<T> null((size_t)nPerms - 1);
    for (long k = 1; k < nPerms; k++) null[k - 1] = of(k);
    return frog::NullDistribution<T>(std::move(null));
}

void write_maps(Output &out, const Inputs &in, Fit &fit)
{
    for (size_t j = 0; j < in.p; j++) out.volume("beta_" + std::to_string(j) + ".nii.gz", FROG_V_F32, fit.beta.data() + j * in.total);
    out.volume("sigma.nii.gz", FROG_V_F32, fit.sigma.data());
    out.volume("count.nii.gz", FROG_V_U16, fit.count.data());
    for (size_t c = 0; c < in.n_c; c++) out.volume("t_" + std::to_string(c) + ".nii.gz", FROG_V_F32, fit.t.data() + c * in.total);
}

// glm.csv's last two columns, per contrast: NaN and 0 without permutations
struct Verdicts {
    std::vector<double> threshold;
    std::vector<uint64_t> beyond;
};

// maxt.csv and fwe_p_<c>
void write_fwe(Output &out, const Options &o, const Inputs &in, const Fit &fit, Verdicts &verdicts)
{
    const size_t n_c = in.n_c, total = in.total;
    const long nPerms = o.nPerms;
    std::ofstream csv(out.path("maxt.csv"));
    csv << "permutation,contrast,max,min\n";
    for (long k = 0; k < nPerms; k++)
        for (size_t c = 0; c < n_c; c++) csv << k << "," << c << "," << csv_float(fit.maxT[k * n_c + c]) << "," << csv_float(fit.minT[k * n_c + c]) << "\n";
    out.close(csv, "maxt.csv");
    std::vector<float> pmap(total);
    for (size_t c = 0; c < n_c; c++) {
        const auto null = null_of<float>(nPerms, [&](long k) {
            const float row[2] = { fit.maxT[k * n_c + c], -fit.minT[k * n_c + c] };
            return frog::sides_max(row, o.sides());
        });
        verdicts.threshold[c] = null.threshold_p05();
        for (size_t v = 0; v < total; v++) {
            float value = fit.t[c * total + v];
            if (o.twoSided == 1) value = std::fabs(value);
            pmap[v] = 1.0f;
            if (fit.marker[v] == -1.0f || std::isnan(value)) continue;
            const auto verdict = null.test(value);
            pmap[v] = verdict.p;
            if (verdict.significant) verdicts.beyond[c]++;
        }
        out.volume("fwe_p_" + std::to_string(c) + ".nii.gz", FROG_V_F32, pmap.data());
    }
}

// maxextent.csv, clusters.csv, clusters_<c> and cluster_p_<c>
void write_clusters(Output &out, const Options &o, const Inputs &in, const Fit &fit, Clusters &got)
{
    const size_t n_c = in.n_c, total = in.total;
    const long nPerms = o.nPerms;
    std::ofstream csv(out.path("maxextent.csv")), table(out.path("clusters.csv"));
    csv << "permutation,contrast,extent\n";
    table << "contrast,cluster,sign,voxels,peak_t,peak_x,peak_y,peak_z,p_fwe\n";
    auto nullExtent = [&](long k, size_t c) { return frog::sides_max(got.extent.data() + ((size_t)k * n_c + c) * o.sides(), o.sides()); };
    for (long k = 0; k < nPerms; k++)
        for (size_t c = 0; c < n_c; c++) csv << k << "," << c << "," << nullExtent(k, c) << "\n";
    out.close(csv, "maxextent.csv");
    std::vector<float> pmap(total);
    for (size_t c = 0; c < n_c; c++) {
        const size_t found = got.sign[c].size();
        const uint32_t *labels = got.labels.data() + c * total;
        const float *t = fit.t.data() + c * total;
        std::vector<uint64_t> voxels(found + 1, 0);
        std::vector<size_t> peak(found + 1, total);
        for (size_t v = 0; v < total; v++) {
            const uint32_t l = labels[v];
            if (!l) continue;
            voxels[l]++;
            if (peak[l] == total || std::fabs(t[v]) > std::fabs(t[peak[l]])) peak[l] = v;
        }
        const auto null = null_of<uint32_t>(nPerms, [&](long k) { return nullExtent(k, c); });
        std::vector<float> pOf(found + 1, 1.0f);
        for (size_t l = 1; l <= found; l++) {
            pOf[l] = null.p((uint32_t)voxels[l]);
            table << c << "," << l << "," << got.sign[c][l - 1] << "," << voxels[l] << ",";
            frog::write_peak(table, t, peak[l], in.grid.dims);
            table << "," << csv_float(pOf[l]) << "\n";
        }
        for (size_t v = 0; v < total; v++) pmap[v] = pOf[labels[v]];
        out.volume("clusters_" + std::to_string(c) + ".nii.gz", FROG_V_I32, got.labels.data() + c * total);
        out.volume("cluster_p_" + std::to_string(c) + ".nii.gz", FROG_V_F32, pmap.data());
    }
    out.close(table, "clusters.csv");
}

// maxtfce.csv, tfce.csv, tfce_<c> and tfce_p_<c>
void write_tfce(Output &out, const Options &o, const Inputs &in, Enhanced &got)
{
    const size_t n_c = in.n_c, total = in.total;
    const long nPerms = o.nPerms;
    std::ofstream csv(out.path("maxtfce.csv")), table(out.path("tfce.csv"));
    csv << "permutation,contrast,max_tfce\n";
    table << "contrast,peak_tfce,peak_x,peak_y,peak_z,threshold_p05,voxels_p05\n";
    auto nullTfce = [&](long k, size_t c) { return frog::sides_max(got.max.data() + ((size_t)k * n_c + c) * o.sides(), o.sides()); };
    for (long k = 0; k < nPerms; k++)
        for (size_t c = 0; c < n_c; c++) csv << k << "," << c << "," << csv_float(nullTfce(k, c)) << "\n";
    out.close(csv, "maxtfce.csv");
    std::vector<float> pmap(total);
    for (size_t c = 0; c < n_c; c++) {
        const auto null = null_of<float>(nPerms, [&](long k) { return nullTfce(k, c); });
        const float *map = got.map.data() + c * total;
        uint64_t past = 0;
        size_t peak = total;
        for (size_t v = 0; v < total; v++) {
            const float value = std::fabs(map[v]);
            pmap[v] = 1.0f;
            if (value == 0.0f) continue;
            const auto verdict = null.test(value);
            pmap[v] = verdict.p;
            if (verdict.significant) past++;
            if (peak == total || value > std::fabs(map[peak])) peak = v;
        }
        table << c << ",";
        frog::write_peak(table, map, peak, in.grid.dims);
        table << "," << csv_float((float)null.threshold_p05()) << "," << past << "\n";
        out.volume("tfce_" + std::to_string(c) + ".nii.gz", FROG_V_F32, got.map.data() + c * total);
        out.volume("tfce_p_" + std::to_string(c) + ".nii.gz", FROG_V_F32, pmap.data());
    }
    out.close(table, "tfce.csv");
}

void write_glm_csv(const Output &out, const Options &o, const Inputs &in, const Fit &fit, const Verdicts &verdicts)
{
    const size_t total = in.total;
    std::ofstream csv(out.path("glm.csv"));
    csv << "contrast,fit_voxels,peak_t,peak_x,peak_y,peak_z,threshold_p05,voxels_p05\n";
    for (size_t c = 0; c < in.n_c; c++) {
        const float *t = fit.t.data() + c * total;
        uint64_t fitted = 0;
        size_t peak = total;
        for (size_t v = 0; v < total; v++) {
            const float value = t[v];
            if (fit.marker[v] == -1.0f || std::isnan(value)) continue;
            fitted++;
            const float best = peak < total ? t[peak] : 0.0f;
            if (peak == total || (o.twoSided == 1 ? std::fabs(value) > std::fabs(best) : value > best)) peak = v;
        }
        csv << c << "," << fitted << ",";
        frog::write_peak(csv, t, peak, in.grid.dims);
        csv << "," << csv_float((float)verdicts.threshold[c]) << "," << verdicts.beyond[c] << "\n";
    }
    out.close(csv, "glm.csv");
}

} // namespace

int main(int argc, char *argv[])
{
    PhaseTimes times;
    const Options o = parse_options(argc, argv);
    if (o.positional.size() != 3) {
        std::cout << "Usage : GroupStats bbox.json spacing design.csv [-c contrasts.csv] [-td transformsDir] [-o outDir] "
                     "[-v jacobian|logjacobian|images] [-vl volumes.txt] [-ml masks.txt] [-m regionMask] [-mc minCount] [-sf sigmaFloor] "
                     "[-f fill] [-np nPerms] [-ps seed] [-pc columns] [-pf 1] [-two 1] [-ct threshold] [-cc 6|18|26] [-tf 1] [-tfd dh] [-tfe 0.5|1] [-tfh 1|2] "
                     "[-s fwhm_mm] [-rp planes] [-dev n]\n-tf 1: threshold-free cluster enhancement in steps of dh (default 0.1); a statistic beyond 255 * dh "
                     "saturates there" << std::endl;
        return 1;
    }

    // ---- everything is checked before the first output: the options, the inputs, and that the sinks fit the device
    Inputs in;
    check_options(o, in);
    load_model(o, in);
    load_images(o, in);
    frog_clusters *sink = nullptr;
    if (o.clusterTest && frog_clusters_create(&in.grid, (uint32_t)o.nPerms, (uint32_t)in.n_c, o.twoSided == 1, (float)o.clusterThreshold, o.connectivity, o.device, &sink))
        die(frog_last_error());
    frog_tfce *enhance = nullptr;
    if (o.tfceTest && frog_tfce_create(&in.grid, (uint32_t)o.nPerms, (uint32_t)in.n_c, o.twoSided == 1, (float)o.tfceStep, o.tfceE, o.tfceH, o.connectivity, o.device, &enhance))
        die(frog_last_error());
    begin_output(o.outDir, in.n, "images", in.grid);

    // ---- the device's work: the slabs, then each sink's read-out
    auto t0 = clk::now();
    Plan plan;
    set_up(o, in, plan);
    times.setup_s = seconds(t0);
    Fit fit;
    fit_slabs(o, in, plan, sink, enhance, fit, times);
    Clusters clusters;
    Enhanced enhanced;
    if (sink) read_clusters(sink, o, in, clusters, times);
    if (enhance) read_tfce(enhance, o, in, enhanced, times);

    // ---- the files
    t0 = clk::now();
    Output out{ o.outDir, in.grid };
    Verdicts verdicts{ std::vector<double>(in.n_c, NAN), std::vector<uint64_t>(in.n_c, 0) };
    write_maps(out, in, fit);
    if (o.nPerms) write_fwe(out, o, in, fit, verdicts);
    if (o.clusterTest) write_clusters(out, o, in, fit, clusters);
    if (o.tfceTest) write_tfce(out, o, in, enhanced);
    write_glm_csv(out, o, in, fit, verdicts);
    times.write_s += seconds(t0);
    times.print(fit.read_s, in.images || !in.masks.empty() ? fit.threads : 0);
    return 0;
}
