# builds the dump of plan_flat_range (csrc/range_plan.h), host compiler only:  make -C tests/cpp -f range_plan.mk [OUT=path]
ROOT := ../..
CXX  ?= g++
CSRC := $(ROOT)/vector_line_quantization_amd/csrc
OUT  ?= range_plan_dump
all: $(OUT)
$(OUT): range_plan_dump.cpp $(CSRC)/range_plan.h $(CSRC)/flat_plan.h $(CSRC)/scan_plan.h
	$(CXX) -std=c++17 -O1 -Wall -I$(CSRC) $< -o $@
clean:
	rm -f range_plan_dump
.PHONY: all clean
