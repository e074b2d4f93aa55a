// Example, host side: a batch target run through the reference's own template surface on one MI355X.
//
// The Calculator is still a reference Calculator (`double calcLogPostProb(double*)`, /root/reference/MCMCpp/Movers/
// StretchMove.h:42-54), used for the initial auxValues.  What makes it a batch target is
//   static const int hipCalcId = MCMC::Device::BatchCalcId;
//   int hipBatchLogPostProb(const double* dProposals, long long count, int numParams, double* dLogp, void* hipStream);
// which the sampler calls once per half-step with the W/2 proposals in device memory (count = W/2): here it launches the
// kernel of examples/batch_calculator_device.hip, compiled with hipcc into libbatch_calculator.so.
//
//   g++ -std=c++11 -O2 -I include/MCMCpp -I include examples/batch_calculator.cpp -L <dir of libbatch_calculator.so>
//       -lbatch_calculator -L mcmcpp_amd -lmcmcpp_hip -Wl,-rpath,... -o batch_calculator
//   ./batch_calculator W D steps interval seed init.bin chain_out.bin
//
// init.bin: W*D doubles.  The program samples the isotropic Gaussian twice with ParallelEnsembleSampler -- through the
// batch target and through the library's built-in Device::IsoGaussian -- and checks that the chains and acceptance counts
// are identical.  chain_out.bin receives the batch target's chain (initial placement first); the last line printed is
// "accepted <accepted>/<total>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "Device/Calculators.h"
#include "Movers/StretchMove.h"
#include "ParallelEnsembleSampler.h"

extern "C" int iso_gaussian_batch_logp(const double* dProposals, long long count, int numParams, double* dLogp, void* hipStream);

class BatchIsoGaussian
{
public:
    static const int hipCalcId = MCMC::Device::BatchCalcId;
    explicit BatchIsoGaussian(int numParams) : host(numParams) {}
    double calcLogPostProb(double* x) { return host.calcLogPostProb(x); }
    int hipBatchLogPostProb(const double* dProposals, long long count, int numParams, double* dLogp, void* hipStream)
    {
        return iso_gaussian_batch_logp(dProposals, count, numParams, dLogp, hipStream);
    }

private:
    MCMC::Device::IsoGaussian<double> host;  // the host twin computes the same bits
};

template <class Calc>
static std::vector<double> sample(Calc calc, int W, int D, int steps, int interval, int seed, const std::vector<double>& init,
                                  unsigned long long* accepted, unsigned long long* total)
{
    typedef MCMC::Mover::StretchMove<double, Calc> Mover;
    Mover mover(D, 0, calc);
    MCMC::ParallelEnsembleSampler<double, Mover> sampler(seed, 4, W, D, mover);
    sampler.setSamplingMode(interval, 0);
    std::vector<double> pos(init), aux(W);
    for (int w = 0; w < W; ++w) aux[w] = calc.calcLogPostProb(&pos[(size_t)w * D]);
    sampler.setInitialWalkerPos(pos.data(), aux.data());
    sampler.runMCMC(steps);
    *accepted = sampler.getAcceptedSteps();
    *total = sampler.getTotalSteps();
    std::vector<double> chain;
    for (auto it = sampler.getStepIttBegin(); it != sampler.getStepIttEnd(); ++it) chain.insert(chain.end(), *it, *it + (size_t)W * D);
    return chain;
}

int main(int argc, char** argv)
{
    if (argc < 8)
    {
        std::fprintf(stderr, "usage: batch_calculator W D steps interval seed init.bin chain_out.bin\n");
        return 2;
    }
    const int W = std::atoi(argv[1]), D = std::atoi(argv[2]), steps = std::atoi(argv[3]), interval = std::atoi(argv[4]), seed = std::atoi(argv[5]);
    std::vector<double> init((size_t)W * D);
    FILE* fp = std::fopen(argv[6], "rb");
    if (!fp || std::fread(init.data(), sizeof(double), init.size(), fp) != init.size())
    {
        std::fprintf(stderr, "cannot read %s\n", argv[6]);
        return 2;
    }
    std::fclose(fp);

    unsigned long long accBatch = 0, totBatch = 0, accBuiltin = 0, totBuiltin = 0;
    const std::vector<double> batch = sample(BatchIsoGaussian(D), W, D, steps, interval, seed, init, &accBatch, &totBatch);
    const std::vector<double> builtin = sample(MCMC::Device::IsoGaussian<double>(D), W, D, steps, interval, seed, init, &accBuiltin, &totBuiltin);
    const bool same = batch.size() == builtin.size() && std::memcmp(batch.data(), builtin.data(), sizeof(double) * batch.size()) == 0 &&
                      accBatch == accBuiltin && totBatch == totBuiltin;
    std::printf("batch target against the built-in isotropic Gaussian: %s\n", same ? "identical chains" : "CHAINS DIFFER");
    fp = std::fopen(argv[7], "wb");
    if (!fp || std::fwrite(batch.data(), sizeof(double), batch.size(), fp) != batch.size()) return 2;
    std::fclose(fp);
    std::printf("accepted %llu/%llu\n", accBatch, totBatch);
    return same ? 0 : 1;
}
