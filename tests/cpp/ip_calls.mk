# builds tests/cpp/ref_drivers/ip_calls (reference headers, linked like the reference's drivers: the interposer in
# front of the reference's library) after `make -C tests/cpp ref_drivers` has built the interposer:
#   make -C tests/cpp -f ip_calls.mk
ROOT := ../..
CXX  ?= g++
REF ?= /root/reference
RD := ref_drivers
MKL_LINK := -Wl,--no-as-needed /opt/conda/lib/libmkl_gf_lp64.so /opt/conda/lib/libmkl_gnu_thread.so /opt/conda/lib/libmkl_core.so -lgomp -lpthread -lm -ldl
RPATHS := -Wl,-rpath,'$$ORIGIN' -Wl,-rpath,'$$ORIGIN/../../../oracle/_ref' -Wl,-rpath,'$$ORIGIN/../../../vector_line_quantization_amd/csrc' -Wl,-rpath,/opt/rocm/lib
all: $(RD)/ip_calls
$(RD)/ip_calls: ip_calls.cpp $(RD)/libvlq_interpose.so
	$(CXX) -std=c++11 -O2 -w -fopenmp -DFINTEGER=int -I$(REF) $< -o $@ -L$(RD) -lvlq_interpose -L$(ROOT)/oracle/_ref -lfaiss_ref \
	    -L$(ROOT)/vector_line_quantization_amd/csrc -lvlq_ivfpq $(RPATHS) $(MKL_LINK)
.PHONY: all
