// tests/cpp/blstm_test.cpp -- drives include/klstm_blstm.hpp (the bidirectional layer) for tests/test_blstm.py (host-only modes, no
// GPU) and tests/test_blstm_gpu.py.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>

#include "../../include/klstm_blstm.hpp"

using namespace klstm_kaldi;

static std::vector<float> read_raw(const std::string &path) {
  std::ifstream f(path, std::ios::binary);
  if (!f) KLSTM_ERR("cannot open " << path);
  f.seekg(0, std::ios::end);
  const size_t n = (size_t)f.tellg() / sizeof(float);
  f.seekg(0);
  std::vector<float> v(n);
  f.read(reinterpret_cast<char *>(v.data()), n * sizeof(float));
  return v;
}
static void write_raw(const std::string &path, const std::vector<float> &v) {
  std::ofstream f(path, std::ios::binary);
  f.write(reinterpret_cast<const char *>(v.data()), v.size() * sizeof(float));
}
static std::vector<int32> parse_ints(const std::string &csv) {
  std::vector<int32> v;
  std::stringstream ss(csv);
  std::string tok;
  while (std::getline(ss, tok, ',')) if (!tok.empty()) v.push_back(atoi(tok.c_str()));
  return v;
}
static LstmProjectedStreams *load_model(const std::string &path) {
  std::ifstream f(path, std::ios::binary);
  if (!f) KLSTM_ERR("cannot open " << path);
  const bool binary = InitKaldiInputStream(f);
  LstmProjectedStreams *c = ReadLstmComponent(f, binary);
  if (!c) KLSTM_ERR("no component in " << path);
  return c;
}
static BLstmProjectedStreams *load_blstm(const char *fwd, const char *bwd) {
  std::unique_ptr<LstmProjectedStreams> f(load_model(fwd)), b(load_model(bwd));
  LstmProjectedStreams *fp = f.release(), *bp = b.release();
  return new BLstmProjectedStreams(fp, bp);              // owns both from its first member on, also when it throws
}

int main(int argc, char **argv) {
  try {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "shape" && argc == 4) {
      // shape <fwd_model> <bwd_model>          construction only (host): "OK in out params" or the error
      std::unique_ptr<BLstmProjectedStreams> l(load_blstm(argv[2], argv[3]));
      std::cout << "OK " << l->InputDim() << " " << l->OutputDim() << " " << l->NumParams() << "\n";
    } else if (mode == "write" && argc == 4) {
      // write <fwd_model> <bwd_model>          Nnet::Write of a net holding the layer (host): refused
      Nnet nnet;
      nnet.AppendComponent(new BLstmLayer(load_blstm(argv[2], argv[3])));
      std::ostringstream os;
      nnet.Write(os, true);
      std::cout << "OK\n";
    } else if (mode == "seqlens" && argc == 5) {
      // seqlens <fwd_model> <bwd_model> <len,len,...>      SetSeqLengths' host checks (the device copy needs a GPU)
      std::unique_ptr<BLstmProjectedStreams> l(load_blstm(argv[2], argv[3]));
      l->SetSeqLengths(parse_ints(argv[4]));
      std::cout << "OK\n";
    } else if (mode == "layer" && argc == 13) {
      // layer <fwd_model> <bwd_model> <x_raw> <od_raw> <len,len,...> <lr> <momentum> <fuse 0/1> <in_diff 0/1> <minibatches> <out_prefix>
      // BLstmProjectedStreams alone: per minibatch SetSeqLengths, PropagateFnc, BackpropagateFnc (+ Update, lr > 0); the same x / od
      // every minibatch.  Writes <prefix>out.raw, in_diff.raw (last minibatch), params.raw (after the last Update)
      std::unique_ptr<BLstmProjectedStreams> l(load_blstm(argv[2], argv[3]));
      const std::vector<float> x = read_raw(argv[4]), od = read_raw(argv[5]);
      const std::vector<int32> lens = parse_ints(argv[6]);
      const float lr = (float)atof(argv[7]);
      NnetTrainOptions o;
      o.learn_rate = lr; o.momentum = (float)atof(argv[8]);
      l->SetTrainOptions(o);
      const bool fuse = atoi(argv[9]) != 0, want_id = atoi(argv[10]) != 0;
      const int nmb = atoi(argv[11]);
      const std::string pre = argv[12];
      const int32 I = l->InputDim(), O = l->OutputDim(), rows = (int32)(x.size() / I);
      DeviceMatrix xd, odd, out, id;
      xd.CopyFromHost(x.data(), rows, I);
      odd.CopyFromHost(od.data(), rows, O);
      out.Resize(rows, O);
      id.Resize(rows, I);
      for (int k = 0; k < nmb; k++) {
        l->SetSeqLengths(lens);
        MatrixView ov = out.View(), idv = id.View();
        l->PropagateFnc(xd.View(), &ov);
        l->SetUpdateFollows(fuse);
        l->BackpropagateFnc(xd.View(), ov, odd.View(), want_id ? &idv : nullptr);
        if (lr > 0) l->Update(xd.View(), odd.View());
        l->SetUpdateFollows(false);
      }
      KCheck(klstm_stream_synchronize(nullptr));
      std::vector<float> h;
      out.CopyToHost(&h); write_raw(pre + "out.raw", h);
      id.CopyToHost(&h); write_raw(pre + "in_diff.raw", h);
      l->GetParams(&h); write_raw(pre + "params.raw", h);
      std::cout << "OK\n";
    } else if (mode == "nnet" && argc == 12) {
      // nnet <fwd_model> <bwd_model> <W_raw> <b_raw> <x_raw> <od_raw> <len,len,...> <lr> <momentum> <out_prefix>
      // Nnet of Transmit -> BLstm -> Affine -> Softmax: SetSeqLengths, Propagate, Backpropagate(od = the softmax input's diff).
      // Writes <prefix>out.raw (the softmax output), blstm.raw (its parameters), affine.raw (W then b, after the Update)
      Nnet nnet;
      std::unique_ptr<BLstmProjectedStreams> l(load_blstm(argv[2], argv[3]));
      const int32 I = l->InputDim(), O = l->OutputDim();
      BLstmLayer *bl = new BLstmLayer(l.release());
      const std::vector<float> W = read_raw(argv[4]), b = read_raw(argv[5]), x = read_raw(argv[6]), od = read_raw(argv[7]);
      const int32 P = (int32)b.size(), rows = (int32)(x.size() / I);
      AffineLayer *aff = new AffineLayer(O, P);
      aff->SetParams(W, b);
      nnet.AppendComponent(new TransmitLayer(I, I));
      nnet.AppendComponent(bl);
      nnet.AppendComponent(aff);
      nnet.AppendComponent(new SoftmaxLayer(P, P));
      NnetTrainOptions o;
      o.learn_rate = (float)atof(argv[9]); o.momentum = (float)atof(argv[10]);
      nnet.SetTrainOptions(o);
      const std::string pre = argv[11];
      DeviceMatrix xd, odd, out;
      xd.CopyFromHost(x.data(), rows, I);
      odd.CopyFromHost(od.data(), rows, P);
      nnet.SetSeqLengths(parse_ints(argv[8]));
      nnet.Propagate(xd.View(), &out);
      nnet.Backpropagate(odd.View(), nullptr);
      KCheck(klstm_stream_synchronize(nullptr));
      std::vector<float> h, hb;
      out.CopyToHost(&h); write_raw(pre + "out.raw", h);
      bl->GetParams(&h); write_raw(pre + "blstm.raw", h);
      aff->HostParams(&h, &hb); h.insert(h.end(), hb.begin(), hb.end()); write_raw(pre + "affine.raw", h);
      std::cout << "OK\n";
    } else {
      std::cerr << "usage: blstm_test shape|write|seqlens|layer|nnet ...\n";
      return 2;
    }
  } catch (const std::exception &e) {
    std::cout << "ERROR " << e.what() << "\n";
    return 1;
  }
  return 0;
}
