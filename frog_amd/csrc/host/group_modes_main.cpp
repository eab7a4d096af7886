// GroupModes: how does a registered group vary as a whole -- the statistical deformation model of Rueckert, Frangi and Schnabel
// (IEEE TMI 2003): a principal component analysis of the images' values in the group's space (frog_modes, include/frog_chain.h,
// which states the arithmetic).
//   GroupModes bbox.json spacing [-td transformsDir] [-o outDir] [-v displacement|logjacobian|jacobian|images] [-vl volumes.txt]
//              [-ml masks.txt] [-m region] [-k nModes] [-nl 0|1] [-ms s] [-f fill] [-rp planes] [-dev n]
// The grid is DummyVolumeGenerator's (frog_bbox_grid).  Image i is <transformsDir>/<i>.json (default "transforms"; the images
// are counted from 0 until a file is missing), inverted as AverageImage inverts it.  -nl 1 drops the linear links from every
// inverted chain before it is sampled: the deformable part alone, the usual pose-free model.
// -v (default displacement): the value of image i at a grid voxel.  displacement: where the chain takes the voxel, minus the
// voxel, in mm (3 components; what TransformField writes).  logjacobian, jacobian and images: as in GroupStats (1 component);
// -vl, -ml and -m as there.  A voxel is in the SUPPORT where -m (if given) is non-zero and every image takes part.
// -k nModes: the modes kept, default min(N - 1, 8).  With G = gram / (N - 1) and its eigenpairs (lambda_k, e_k), mode k is the
// sum over the images of e_ik / sqrt(N - 1) times the centred image: a field in units per standard deviation.
// Outputs in outDir: mean.nii.gz and mode_<k>.nii.gz (FLOAT32, 3 or 1 components; -f, default 0, outside the support),
// support.nii.gz (UINT8), modes.csv: mode,eigenvalue,rms,share,cumulative -- rms = sqrt(lambda / (support voxels x components)),
// the modes' rms per value; share = lambda / the sum of all N eigenvalues -- and scores.csv: image,score_<k>...,distance,
// distance_robust_z -- score_k = sqrt(N - 1) e_ik in standard deviations, distance the norm of the kept scores, and its robust z
// across the group by quality.csv's rule: an image far out in the model space is an outlier.  Doubles as %.17g.
// -ms s (displacement only; default 0: none): mean_field.nii.gz with mean.json, and per kept mode mode_<k>_plus.nii.gz,
// mode_<k>_minus.nii.gz with mode_<k>_plus.json and mode_<k>_minus.json: one-entry frogDisplacementField transforms of
// mean and mean +- s mode_k (f32: p = s * mode, mean +- p), 0 outside the support, which every tool that takes -t reads.
// The device holds slabs of frog_modes_planes z-planes, or -rp planes if that is fewer.  One slab: the images are added once.
// More: TWO passes, every image added twice -- the Gram matrix of all slabs in ascending order (the order the stated sums
// need), the eigen-solve on the host, then per slab the adds again and the projection.  The slab count is printed and changes
// no bit of any file.  Every input is checked before anything is written.
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

// the median of a non-empty list: the middle value, or the mean of the middle two (as quality.csv's)
double median(std::vector<double> v)
{
    std::sort(v.begin(), v.end());
    const size_t n = v.size();
    return n % 2 ? v[n / 2] : (v[n / 2 - 1] + v[n / 2]) / 2.0;
}

struct Options {
    std::vector<std::string> positional;
    std::string transformsDir = "transforms", outDir = ".", valueName = "displacement", volumeList, maskList, regionPath;
    long nModes = 0, planesOption = 0;
    int device = 0, noLinear = 0;
    double modeSd = 0;
    float fill = 0;
    bool modesGiven = false, planesGiven = false;
};

Options parse_options(int argc, char *argv[])
{
    Options o;
    int a = positional_arguments(argc, argv, 1, { "-td", "-o", "-v", "-vl", "-ml", "-m", "-k", "-nl", "-ms", "-f", "-rp", "-dev" }, o.positional);
    for (; a < argc; a += 2) {
        const char *key = argv[a], *value = a + 1 < argc ? argv[a + 1] : "";
        if (std::strcmp(key, "-td") == 0) o.transformsDir = value;
        else if (std::strcmp(key, "-o") == 0) o.outDir = value;
        else if (std::strcmp(key, "-v") == 0) o.valueName = value;
        else if (std::strcmp(key, "-vl") == 0) o.volumeList = value;
        else if (std::strcmp(key, "-ml") == 0) o.maskList = value;
        else if (std::strcmp(key, "-m") == 0) o.regionPath = value;
        else if (std::strcmp(key, "-k") == 0) { o.nModes = atol(value); o.modesGiven = true; }
        else if (std::strcmp(key, "-nl") == 0) o.noLinear = atoi(value);
        else if (std::strcmp(key, "-ms") == 0) o.modeSd = atof(value);
        else if (std::strcmp(key, "-f") == 0) o.fill = (float)atof(value);
        else if (std::strcmp(key, "-rp") == 0) { o.planesOption = atol(value); o.planesGiven = true; }
        else if (std::strcmp(key, "-dev") == 0) o.device = atoi(value);
        else die(std::string("unknown option ") + key);
    }
    return o;
}

// what the checks load and work out
struct Inputs {
    bool images = false, logMode = false;
    uint32_t components = 3;
    size_t n = 0, keep = 0;
    std::vector<std::string> volumes, masks;
    frog_volume grid;
    size_t plane = 0, total = 0;
    ChainArguments transforms;
    std::vector<std::vector<frog_chain_link>> inverse;
    std::vector<frog_volume> supports;
    std::vector<uint8_t> region;
};

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

void load_inputs(const Options &o, Inputs &in)
{
    const bool displacement = o.valueName == "displacement";
    in.images = o.valueName == "images";
    in.logMode = o.valueName == "logjacobian";
    if (!displacement && !in.images && !in.logMode && o.valueName != "jacobian")
        die("-v takes displacement, logjacobian, jacobian or images, not '" + o.valueName + "'");
    in.components = displacement ? 3 : 1;
    if (in.images && o.volumeList.empty()) die("-v images needs the volumes: -vl volumes.txt");
    if (o.noLinear != 0 && o.noLinear != 1) die("-nl takes 0 or 1");
    if (!(o.modeSd >= 0.0) || !std::isfinite((float)o.modeSd)) die("-ms takes a number of standard deviations that is finite and not negative");
    if (o.modeSd > 0.0 && !displacement) die("-ms writes displacement fields: it needs -v displacement");
    if (o.planesGiven && o.planesOption < 1) die("-rp takes a number of planes, at least 1");
    if (frog_bbox_grid(o.positional[0].c_str(), atof(o.positional[1].c_str()), &in.grid))
        die("cannot read a bounding box from " + o.positional[0] + " (or spacing " + o.positional[1] + " is not positive)");
    if (!o.volumeList.empty() && !read_list(o.volumeList, in.volumes)) die("cannot read the volume list " + o.volumeList);
    if (!o.maskList.empty() && !read_list(o.maskList, in.masks)) die("cannot read the mask list " + o.maskList);
    // the images: those of the lists, or transforms/0.json, 1.json ... until one is missing
    size_t n = !in.volumes.empty() ? in.volumes.size() : in.masks.size();
    if (!n)
        while (std::ifstream(o.transformsDir + "/" + std::to_string(n) + ".json")) n++;
    in.n = n;
    if (n < 2) die("at least two images are needed: " + std::to_string(n) + " found in " + o.transformsDir);
    if (n > FROG_MODES_MAX_IMAGES) die("at most " + std::to_string(FROG_MODES_MAX_IMAGES) + " images");
    if (!in.volumes.empty() && !in.masks.empty() && in.masks.size() != n)
        die(o.maskList + " holds " + std::to_string(in.masks.size()) + " masks for " + std::to_string(n) + " volumes");
    in.keep = o.modesGiven ? (size_t)std::max(0l, o.nModes) : std::min<size_t>(n - 1, 8);
    if (o.modesGiven && (o.nModes < 1 || (size_t)o.nModes > n)) die("-k takes 1 to " + std::to_string(n) + " modes");
    in.inverse = inverse_transforms(in.transforms, o.transformsDir, n);
    if (o.noLinear == 1)
        for (auto &links : in.inverse)
            links.erase(std::remove_if(links.begin(), links.end(), [](const frog_chain_link &l) { return l.type == FROG_T_LINEAR; }), links.end());
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

struct Work {
    std::vector<frog_chain *> chains;
    uint32_t planes = 0;
    double read_s = 0;
    int threads = 1;
    size_t window = 1;
};

// a slab's accumulator with every image's values, in the order of the images
frog_modes *filled_slab(const Options &o, const Inputs &in, Work &work, uint32_t first, uint32_t count_planes, PhaseTimes &times)
{
    frog_modes *acc = nullptr;
    auto t0 = clk::now();
    if (frog_modes_create(&in.grid, first, count_planes, (uint32_t)in.n, in.components, o.device, &acc)) die(frog_last_error());
    times.device_s += seconds(t0);
    std::unique_ptr<frog::VolumeStream> stream(in.images ? new frog::VolumeStream(in.volumes, work.threads, work.window) : nullptr);
    std::unique_ptr<frog::VolumeStream> maskStream(in.masks.empty() ? nullptr : new frog::VolumeStream(in.masks, work.threads, work.window));
    for (size_t i = 0; i < in.n; i++) {
        double waited = 0;
        const frog_volume *mask = nullptr;
        if (maskStream) {
            frog::VolumeStream::Item &m = maskStream->get(i, &waited);
            times.waited_s += waited;
            if (!m.file) die("cannot read mask " + in.masks[i]);
            mask = &m.view;
        }
        const frog_volume *support = in.supports.empty() ? nullptr : &in.supports[i];
        if (in.images) {
            frog::VolumeStream::Item &it = stream->get(i, &waited);
            times.waited_s += waited;
            if (!it.file) die("cannot read volume " + in.volumes[i]);
            t0 = clk::now();
            if (frog_modes_add(acc, work.chains[i], &it.view, mask, 1, 0.0)) die(in.volumes[i] + ": " + frog_last_error());
            times.device_s += seconds(t0);
            stream->release(i);
        } else {
            t0 = clk::now();
            if (in.components == 3 ? frog_modes_add_displacement(acc, work.chains[i], support, mask)
                                   : frog_modes_add_jacobian(acc, work.chains[i], support, mask, in.logMode))
                die("transform " + std::to_string(i) + ": " + frog_last_error());
            times.device_s += seconds(t0);
        }
        if (maskStream) maskStream->release(i);
    }
    if (stream) work.read_s += stream->read_seconds();
    if (maskStream) work.read_s += maskStream->read_seconds();
    return acc;
}

struct Output {
    std::string dir;
    frog_volume grid;

    std::string path(const std::string &name) const { return dir + "/" + name; }
    void field(const std::string &name, uint32_t components, const float *values) const
    {
        if (frog_nifti_write(path(name).c_str(), grid.dims, grid.spacing, grid.origin, components, values)) die("cannot write " + path(name));
    }
    void transform(const std::string &name, const std::string &file) const
    {
        std::ofstream out(path(name), std::ios::binary);
        out << "{\"transforms\": [{\"type\": \"frogDisplacementField\", \"file\": \"" << file << "\"}]}\n";
        out.close();
        if (!out) die("cannot write " + path(name));
    }
};

} // namespace

int main(int argc, char *argv[])
{
    PhaseTimes times;
    const Options o = parse_options(argc, argv);
    if (o.positional.size() != 2) {
        std::cout << "Usage : GroupModes bbox.json spacing [-td transformsDir] [-o outDir] [-v displacement|logjacobian|jacobian|images] "
                     "[-vl volumes.txt] [-ml masks.txt] [-m region] [-k nModes] [-nl 0|1] [-ms s] [-f fill] [-rp planes] [-dev n]" << std::endl;
        return 1;
    }
    Inputs in;
    load_inputs(o, in);
    begin_output(o.outDir, in.n, "images", in.grid);

    // ---- the device's work
    auto t0 = clk::now();
    Work work;
    work.chains = create_chains(in.inverse, o.device);
    if (frog_modes_planes(&in.grid, (uint32_t)in.n, in.components, o.device, &work.planes)) die(frog_last_error());
    if (o.planesGiven && (uint64_t)o.planesOption < work.planes) work.planes = (uint32_t)o.planesOption;
    const uint32_t depth = in.grid.dims[2], slabs = (depth + work.planes - 1) / work.planes;
    std::cout << "modes : " << slabs << (slabs == 1 ? " slab of " : " slabs of ") << work.planes << " planes, " << in.components << " components, " << in.keep
              << " modes" << (slabs == 1 ? "" : ", every image is added twice") << std::endl;
    frog::volume_stream_shape(in.n, &work.threads, &work.window);
    if (!in.masks.empty()) work.threads = std::max(1, work.threads / 2);
    times.setup_s = seconds(t0);

    const size_t n = in.n, keep = in.keep, C = in.components, total = in.total;
    std::vector<double> gram(n * (n + 1) / 2, 0.0), values(n), vectors(n * n);
    uint64_t n_support = 0;
    frog_modes *kept = nullptr;
    for (uint32_t first = 0; first < depth; first += work.planes) {
        const uint32_t count_planes = std::min(work.planes, depth - first);
        frog_modes *acc = filled_slab(o, in, work, first, count_planes, times);
        t0 = clk::now();
        if (frog_modes_gram(acc, in.region.empty() ? nullptr : in.region.data() + in.plane * first, gram.data(), &n_support)) die(frog_last_error());
        times.device_s += seconds(t0);
        if (slabs == 1) kept = acc; else frog_modes_destroy(acc);
    }
    if (!n_support) die("the support is empty: no voxel is covered by every image");
    if (frog_modes_eigen((uint32_t)n, gram.data(), (double)(n - 1), values.data(), vectors.data())) die(frog_last_error());
    const double root = std::sqrt((double)(n - 1));
    std::vector<double> weights(keep * n);
    for (size_t e = 0; e < keep * n; e++) weights[e] = vectors[e] / root;

    std::vector<float> mean(total * C), modes(keep * total * C), slabModes;
    std::vector<uint8_t> support(total);
    for (uint32_t first = 0; first < depth; first += work.planes) {
        const uint32_t count_planes = std::min(work.planes, depth - first);
        const size_t at = in.plane * first, slabVoxels = in.plane * count_planes;
        frog_modes *acc = kept ? kept : filled_slab(o, in, work, first, count_planes, times);
        t0 = clk::now();
        slabModes.resize(keep * slabVoxels * C);
        // a mean is never NaN inside the support: NaN as the fill marks the voxels outside it
        if (frog_modes_project(acc, in.region.empty() ? nullptr : in.region.data() + at, (uint32_t)keep, weights.data(), NAN, mean.data() + at * C, slabModes.data()))
            die(frog_last_error());
        times.device_s += seconds(t0);
        frog_modes_destroy(acc);
        for (size_t v = 0; v < slabVoxels; v++) {
            const bool inside = !std::isnan(mean[(at + v) * C]);
            support[at + v] = inside;
            if (inside) continue;
            for (size_t c = 0; c < C; c++) mean[(at + v) * C + c] = o.fill;
            for (size_t k = 0; k < keep; k++)
                for (size_t c = 0; c < C; c++) slabModes[(k * slabVoxels + v) * C + c] = o.fill;
        }
        for (size_t k = 0; k < keep; k++) std::memcpy(modes.data() + (k * total + at) * C, slabModes.data() + k * slabVoxels * C, slabVoxels * C * sizeof(float));
    }
    for (frog_chain *c : work.chains) frog_chain_destroy(c);

    // ---- the files
    t0 = clk::now();
    Output out{ o.outDir, in.grid };
    out.field("mean.nii.gz", in.components, mean.data());
    for (size_t k = 0; k < keep; k++) out.field("mode_" + std::to_string(k) + ".nii.gz", in.components, modes.data() + k * total * C);
    out.grid.dtype = FROG_V_U8;
    out.grid.data = support.data();
    if (frog_volume_write(out.path("support.nii.gz").c_str(), &out.grid)) die("cannot write " + out.path("support.nii.gz"));

    double trace = 0.0;
    for (size_t k = 0; k < n; k++) trace = trace + values[k];
    std::FILE *csv = std::fopen(out.path("modes.csv").c_str(), "w");
    if (!csv) die("cannot write " + out.path("modes.csv"));
    std::fprintf(csv, "mode,eigenvalue,rms,share,cumulative\n");
    const double per_value = (double)n_support * (double)C;
    double cumulative = 0.0;
    for (size_t k = 0; k < keep; k++) {
        const double share = trace > 0.0 ? values[k] / trace : 0.0;
        cumulative = cumulative + share;
        std::fprintf(csv, "%zu,%.17g,%.17g,%.17g,%.17g\n", k, values[k], std::sqrt(std::max(values[k], 0.0) / per_value), share, cumulative);
    }
    if (std::fclose(csv) != 0) die("cannot write " + out.path("modes.csv"));

    std::vector<double> distance(n);
    for (size_t i = 0; i < n; i++) {
        double s = 0.0;
        for (size_t k = 0; k < keep; k++) {
            const double b = root * vectors[k * n + i];
            s = s + b * b;
        }
        distance[i] = std::sqrt(s);
    }
    std::vector<double> spread(distance);
    const double mid = median(spread);
    for (double &x : spread) x = std::fabs(x - mid);
    const double mad = median(spread);
    csv = std::fopen(out.path("scores.csv").c_str(), "w");
    if (!csv) die("cannot write " + out.path("scores.csv"));
    std::fprintf(csv, "image,");
    for (size_t k = 0; k < keep; k++) std::fprintf(csv, "score_%zu,", k);
    std::fprintf(csv, "distance,distance_robust_z\n");
    for (size_t i = 0; i < n; i++) {
        std::fprintf(csv, "%zu,", i);
        for (size_t k = 0; k < keep; k++) std::fprintf(csv, "%.17g,", root * vectors[k * n + i]);
        std::fprintf(csv, "%.17g,%.17g\n", distance[i], mad > 0 ? (distance[i] - mid) / (1.4826 * mad) : 0.0);
    }
    if (std::fclose(csv) != 0) die("cannot write " + out.path("scores.csv"));

    if (o.modeSd > 0.0) {
        const float s = (float)o.modeSd;
        std::vector<float> field(total * 3);
        auto write = [&](const std::string &stem, const float *mode, float sign) {
            for (size_t v = 0; v < total; v++)
                for (size_t c = 0; c < 3; c++) {
                    float f = 0.0f;
                    if (support[v]) {
                        f = mean[v * 3 + c];
                        if (mode) {
                            const float p = s * mode[v * 3 + c];
                            f = sign > 0 ? f + p : f - p;
                        }
                    }
                    field[v * 3 + c] = f;
                }
            out.field(stem + ".nii.gz", 3, field.data());
        };
        write("mean_field", nullptr, 1);
        out.transform("mean.json", "mean_field.nii.gz");
        for (size_t k = 0; k < keep; k++) {
            const std::string stem = "mode_" + std::to_string(k);
            write(stem + "_plus", modes.data() + k * total * 3, 1);
            out.transform(stem + "_plus.json", stem + "_plus.nii.gz");
            write(stem + "_minus", modes.data() + k * total * 3, -1);
            out.transform(stem + "_minus.json", stem + "_minus.nii.gz");
        }
    }
    times.write_s += seconds(t0);
    times.print(work.read_s, in.images || !in.masks.empty() ? work.threads : 0);
    return 0;
}
