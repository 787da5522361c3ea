# builds the dump of plan_hamming_scan (csrc/hamming_plan.h), host compiler only:  make -C tests/cpp -f hamming_plan.mk [OUT=path]
ROOT := ../..
CXX  ?= g++
CSRC := $(ROOT)/vector_line_quantization_amd/csrc
OUT  ?= hamming_plan_dump
all: $(OUT)
$(OUT): hamming_plan_dump.cpp $(CSRC)/hamming_plan.h
	$(CXX) -std=c++17 -O1 -Wall -I$(CSRC) $< -o $@
clean:
	rm -f hamming_plan_dump
.PHONY: all clean
